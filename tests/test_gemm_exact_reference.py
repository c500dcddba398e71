"""The exact-GEMM method (tests/gemm_exact.py) proved on the CPU: for one
CrossNet case and one gemm_nt case the inputs pass assert_exact_inputs and
assert_teeth, fp32 evaluation in another K order equals the fp64 reference
bit for bit, and each deliberate mutation of the reference -- what a subtly
wrong kernel would compute -- changes at least one output element, so
torch.equal against the reference would catch it.  Out-of-range operands
are rejected.  The helpers the GPU tests lean on (guards, report) are
checked too.  No GPU."""
import pytest
import torch

import gemm_exact as X

CPU = "cpu"


# ---------------------------------------------------------------------------
# The two cases, each as a function of its (possibly mutated) pipeline
# ---------------------------------------------------------------------------
class Cross:
    """out = bf16(x0 * (xl W^T + b) + xl) at (B, d) = (257, 320), operands in
    [-4, 4], bias in multiples of 0.25."""
    K_AXIS = 320

    def __init__(self):
        (self.x0, self.xl, self.W, self.b), self.out32, self.lin32 = \
            X.crossnet_case(257, 320, True, CPU)
        self.want = self.out32.to(torch.bfloat16)

    def product(self, rows=slice(None), ks=slice(None)):
        return self.xl.double()[rows, ks] @ self.W.double()[:, ks].t()

    def finish(self, prod, bias=None, round_lin=False, convert=None):
        lin = prod + (self.b if bias is None else bias).double()
        if round_lin:
            lin = lin.float().to(torch.bfloat16).double()
        out = (self.x0.double() * lin + self.xl.double()).float()
        return (convert or (lambda t: t.to(torch.bfloat16)))(out)


class Nt:
    """C = bf16(a b^T + bias) at (M, N, K) = (129, 136, 128), operands in
    [-11, 11] (tests/test_gpu_gemm_exact.py NT_RANGE)."""
    K_AXIS = 128

    def __init__(self):
        g = X.gen(4)
        self.a, self.bm = X.ints(g, (129, 128), 11), X.ints(g, (136, 128), 11)
        self.b = X.quarters(g, 136, 4)
        ref, bound, q = X.gemm_nt_ref(self.a, self.bm, self.b)
        X.assert_exact_inputs(bound, q, bf16=[self.a, self.bm],
                              multiples=[(self.a, 1.0), (self.bm, 1.0), (self.b, 0.25)])
        self.out32 = X.to_f32(ref)
        X.assert_teeth(self.out32)
        self.want = self.out32.to(torch.bfloat16)

    def product(self, rows=slice(None), ks=slice(None)):
        return self.a.double()[rows, ks] @ self.bm.double()[:, ks].t()

    def finish(self, prod, bias=None, round_lin=False, convert=None):
        if round_lin:   # the product rounded to bf16 before the bias is added
            prod = prod.float().to(torch.bfloat16).double()
        out = (prod + (self.b if bias is None else bias).double()).float()
        return (convert or (lambda t: t.to(torch.bfloat16)))(out)


@pytest.fixture(scope="module", params=[Cross, Nt], ids=["crossnet", "gemm_nt"])
def case(request):
    return request.param()


def test_inputs_are_exact_and_have_teeth(case):
    """(the constructors ran assert_exact_inputs and assert_teeth) the
    unmutated pipeline reproduces the reference, and the reference has the
    ties and inexact values that make the rounding mode visible."""
    assert torch.equal(case.finish(case.product()), case.want)
    inexact, tie = X.teeth(case.out32)
    assert inexact >= 0.10 and tie >= 0.05


def test_fp32_in_any_k_order_equals_fp64(case):
    """fp32 arithmetic throughout, K permuted, and K accumulated in chunks
    taken back to front: all equal the fp64 reference bit for bit."""
    lhs = (case.xl if isinstance(case, Cross) else case.a).float()
    rhs = (case.W if isinstance(case, Cross) else case.bm).float()
    want = case.product()
    perm = torch.randperm(case.K_AXIS, generator=X.gen(1))
    assert torch.equal((lhs[:, perm] @ rhs[:, perm].t()).double(), want)
    acc = torch.zeros(lhs.shape[0], rhs.shape[0], dtype=torch.float32)
    for k0 in reversed(range(0, case.K_AXIS, 24)):
        acc = acc + lhs[:, k0:k0 + 24] @ rhs[:, k0:k0 + 24].t()
    assert torch.equal(acc.double(), want)


def _swap_rows(t):
    t = t.clone()
    t[[70, 71]] = t[[71, 70]]          # rows r, r + 1 inside one 64 / 128 / 256 tile
    return t


def _transpose_block(t):
    t = t.clone()
    t[16:32, 48:64] = t[16:32, 48:64].t().clone()
    return t


def _drop_row_tail(case):
    prod = case.product()
    prod[5] = case.product(rows=slice(5, 6), ks=slice(0, case.K_AXIS - 8))[0]
    return prod


def _without_split(case):
    k = case.K_AXIS // 64 // 3 * 64 or 64      # three chunks of whole K steps; the middle one lost
    return case.product() - case.product(ks=slice(k, 2 * k))


MUTATIONS = {
    "one K element dropped":
        lambda c: c.finish(c.product(ks=slice(0, c.K_AXIS - 1))),
    "the last 8-element K vector of one row dropped":
        lambda c: c.finish(_drop_row_tail(c)),
    "truncation instead of round-to-nearest-even":
        lambda c: c.finish(c.product(), convert=X.bf16_truncate),
    "lin rounded to bf16 before use":
        lambda c: c.finish(c.product(), round_lin=True),
    "bias shifted by one column":
        lambda c: c.finish(c.product(), bias=c.b.roll(1)),
    "rows r and r + 1 swapped inside one tile":
        lambda c: _swap_rows(c.finish(c.product())),
    "C transposed within a 16 x 16 block":
        lambda c: _transpose_block(c.finish(c.product())),
    "one split-K partial omitted":
        lambda c: c.finish(_without_split(c)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_changes_the_output(case, name):
    got = MUTATIONS[name](case)
    assert got.dtype == case.want.dtype and got.shape == case.want.shape
    assert not torch.equal(got, case.want), name
    with pytest.raises(AssertionError, match="elements wrong"):
        X.assert_equal(got, case.want, name)


def test_out_of_range_operands_are_rejected():
    """Operands in [-4096, 4096] at K = 3392: most are no bf16 numbers, and
    those that are (multiples of 32 here) still sum past 2^24."""
    g = X.gen(2)
    a = torch.randint(-4096, 4097, (4, 3392), generator=g).double()
    b = torch.randint(-4096, 4097, (8, 3392), generator=g).double()
    bound = a.abs() @ b.abs().t()
    with pytest.raises(AssertionError, match="bf16"):
        X.assert_exact_inputs(bound, 1.0, bf16=[a, b])
    a32, b32 = (a / 32).round() * 32, (b / 32).round() * 32
    with pytest.raises(AssertionError, match="2\\^24"):
        X.assert_exact_inputs(a32.abs() @ b32.abs().t(), 1.0, bf16=[a32, b32])
    with pytest.raises(AssertionError, match="multiple"):
        X.assert_exact_inputs(torch.ones(1, dtype=torch.float64), 0.25,
                              multiples=[(torch.tensor([0.125]), 0.25)])
    # the same K with the tests' range passes
    ok = X.ints(g, (4, 3392), 4)
    X.assert_exact_inputs(ok.double().abs() @ ok.double().abs().t(), 1.0, bf16=[ok])


def test_teeth_rejects_exact_outputs():
    with pytest.raises(AssertionError, match="no teeth"):
        X.assert_teeth(torch.arange(-128, 128, dtype=torch.float32))
    # 257 = 256 + 1 is a tie between 256 and 258; 259 is one too
    assert X.teeth(torch.tensor([257.0, 259.0, 256.0, 258.0])) == (0.5, 0.5)
    assert X.teeth(torch.tensor([513.0, 514.0, 515.0, 516.0])) == (0.75, 0.25)


def test_builders():
    g = X.gen(3)
    m = X.masks(g, (64, 64))
    assert m.dtype == torch.bfloat16
    assert set(m.float().unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 3.0}
    assert bool(torch.signbit(m.float()[m == 0]).any()) and \
        not bool(torch.signbit(m.float()[m == 0]).all())        # both zeros
    q = X.quarters(g, 1000, 4)
    assert q.dtype == torch.float32 and torch.equal((q * 4).round(), q * 4) and q.abs().max() <= 4
    h = X.relu_ints(g, (32, 32), 3)
    assert h.min() == 0 and h.max() == 3
    b = X.coded_b(40, 40)
    assert b.min() == -8 and b.max() == 8 and not torch.equal(b, b.t())
    assert float(b[2, 3]) == (3 * 2 - 5 * 3) % 17 - 8
    perm = torch.randperm(8, generator=g)
    a = X.coded_a(12, 8, perm)
    assert torch.equal(a.float() @ b[:, :8].float().t(),
                       torch.cat([b[:, :8].float().t()[perm], torch.zeros(4, 40)]))


def test_guards_and_report():
    out = X.Guarded(5, 8, torch.bfloat16, CPU, ld=16)
    assert out.view.shape == (5, 8) and out.buf.shape == (5 + X.GUARD_ROWS, 16)
    out.view.zero_()
    out.check()
    out.buf[5, 0] = 1.0                    # a row past the end
    with pytest.raises(AssertionError, match="guard cells overwritten"):
        out.check()
    out.buf[5, 0] = X.SENTINEL
    out.buf[2, 8] = 0.0                    # a column past the end
    with pytest.raises(AssertionError, match="guard cells overwritten"):
        out.check()
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    v = X.nan_padded(t, CPU, ld=8, col_off=2)
    assert torch.equal(v, t) and v.stride(0) == 8
    base = v.as_strided((3 + 253 + X.GUARD_ROWS, 8), (8, 1), 0)
    assert int(base.isnan().sum()) == base.numel() - 12
    want = torch.zeros(300, 300)
    got = want.clone()
    got[255, 127] = 1.0
    rep = X.mismatch_report(got, want, "probe")
    assert "1 of 90000 elements wrong" in rep and "(255, 127): got 1.0, want 0.0" in rep
    assert "mod 256: rows in [255, 255], columns in [127, 127]; 1 on a tile's last row" in rep
    got[0, 0] = float("nan")               # NaNs count as wrong and fail assert_equal
    with pytest.raises(AssertionError, match="2 of 90000"):
        X.assert_equal(got, want, "probe")
    X.assert_equal(torch.tensor([-0.0]), torch.tensor([0.0]))   # values, not bits
