"""Bit-exact checks of the MFMA GEMM kernels on integer-valued operands.

When every operand is a small integer (or a multiple of a small power of two,
the quantum), every product and every partial sum of a GEMM is exactly
representable in fp32, so the fp32 result does not depend on accumulation
order, MFMA shape, split-K, slice order or tile schedule, and the only
rounding left is the final fp32 -> bf16 conversion.  The expected output then
comes from plain fp64 torch and the comparison is torch.equal.

This module holds what the exact tests share (tests/test_gemm_exact_reference.py
on the CPU, tests/test_gpu_gemm_exact.py on the GPU): input builders, the
condition that makes torch.equal legitimate (assert_exact_inputs), the check
that a case exercises the rounding mode (assert_teeth), fp64 references,
guarded buffers, the mismatch report, and the runners that call the C entries
on guarded buffers.  Run as `python tests/gemm_exact.py crossnet` it is the
child process of the test of the CrossNet kernels that an environment
variable selects once per process.  It is not collected as a test."""
import os
import sys

import torch

TWO24 = float(1 << 24)
MASK_VALUES = (-2.0, -1.0, -0.0, 0.0, 1.0, 3.0)
SENTINEL = -777.0          # bf16-exact: what every guard cell holds
ACT_NONE, ACT_RELU, ACT_MASK = 0, 1, 2


# ---------------------------------------------------------------------------
# Input builders (CPU tensors from a CPU torch.Generator)
# ---------------------------------------------------------------------------
def gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def ints(g, shape, r=4, lo=None, dtype=torch.bfloat16):
    """Uniform integers in [lo, r] (lo = -r by default)."""
    lo = -r if lo is None else lo
    return torch.randint(lo, r + 1, tuple(shape), generator=g).to(dtype)


def quarters(g, n, r=4):
    """fp32 multiples of 0.25 in [-r, r]."""
    return torch.randint(-4 * r, 4 * r + 1, (n,), generator=g).to(torch.float32) * 0.25


def masks(g, shape):
    """bf16 values drawn from MASK_VALUES (both zeros, both signs)."""
    vals = torch.tensor(MASK_VALUES, dtype=torch.bfloat16)
    return vals[torch.randint(0, len(MASK_VALUES), tuple(shape), generator=g)]


def relu_ints(g, shape, r=3):
    """Non-negative integers in [0, r], over a third of them exact zeros: the
    output of a ReLU, whose zero pattern is the backward's mask."""
    t = torch.randint(0, r + 1, tuple(shape), generator=g)
    t[torch.rand(tuple(shape), generator=g) < 0.25] = 0
    return t.to(torch.bfloat16)


def coded_b(N, K):
    """B[i][j] = ((3 i - 5 j) mod 17) - 8: no two rows, no two columns and no
    transpose of a block look alike."""
    i = torch.arange(N).reshape(N, 1)
    j = torch.arange(K).reshape(1, K)
    return (((3 * i - 5 * j) % 17) - 8).to(torch.bfloat16)


def coded_a(M, K, perm=None):
    """The identity (perm None) or a row-permuted identity, padded to [M, K]:
    A[i][perm[i]] = 1 for i < min(M, K)."""
    n = min(M, K)
    perm = torch.arange(n) if perm is None else perm
    a = torch.zeros(M, K, dtype=torch.bfloat16)
    a[torch.arange(n), perm] = 1
    return a


# ---------------------------------------------------------------------------
# The conditions
# ---------------------------------------------------------------------------
def assert_exact_inputs(bound, quantum=1.0, bf16=(), multiples=()):
    """What makes torch.equal against the fp64 reference legitimate.
    bound: fp64, per output element the sum of |terms| (products, bias, the
    |x0| factor and the |xl| addend where they apply); quantum: the power of
    two that all terms are multiples of; bf16: the operands the kernel reads
    as bf16; multiples: every operand, checked to be a multiple of its own
    quantum (t, q) so that all terms are multiples of `quantum`.  Below
    2^24 quanta every partial sum, in any order, is an fp32 number."""
    for t in bf16:
        d = t.double()
        if not torch.equal(d.to(torch.bfloat16).double(), d):
            raise AssertionError("an operand is not representable in bf16")
    for t, q in multiples:
        d = t.double() / q
        if not torch.equal(d.round(), d):
            raise AssertionError("an operand is not a multiple of %g" % q)
    top = float(bound.max()) if bound.numel() else 0.0
    if not top < TWO24 * quantum:
        raise AssertionError("sum of |terms| %g reaches 2^24 x %g: fp32 sums would round"
                             % (top, quantum))


def teeth(ref32):
    """(fraction inexact in bf16, fraction exact ties) of an fp32 tensor."""
    ref32 = ref32.float().contiguous()
    inexact = ref32.to(torch.bfloat16).float() != ref32
    tie = (ref32.view(torch.int32) & 0xFFFF) == 0x8000
    n = max(ref32.numel(), 1)
    return float(inexact.sum()) / n, float(tie.sum()) / n


def assert_teeth(ref32, min_inexact=0.10, min_tie=0.05):
    """A bf16 output must exercise the rounding mode: inexact in bf16 on
    >= 10 % of its elements (truncation would show) and an exact tie on
    >= 5 % (round-half-away or half-up would show)."""
    inexact, tie = teeth(ref32)
    if inexact < min_inexact or tie < min_tie:
        raise AssertionError("reference has no teeth: %.1f %% inexact, %.1f %% ties"
                             % (100 * inexact, 100 * tie))


def to_f32(ref64):
    """The fp64 reference as fp32: exact by assert_exact_inputs, and checked.
    A bf16 output is expected to equal this cast to bf16, which torch does
    with round-to-nearest-even."""
    r = ref64.float()
    if not torch.equal(r.double(), ref64):
        raise AssertionError("the fp64 reference is not an fp32 number")
    return r


# ---------------------------------------------------------------------------
# fp64 references: (value, bound, quantum)
# ---------------------------------------------------------------------------
def _q(bias):
    return 1.0 if bias is None else 0.25


def gemm_nt_ref(a, b, bias=None, act=ACT_NONE, mask=None):
    """act(a b^T + bias); ACT_MASK zeroes the result where mask <= 0."""
    v = a.double() @ b.double().t()
    bound = a.double().abs() @ b.double().abs().t()
    if bias is not None:
        v = v + bias.double()
        bound = bound + bias.double().abs()
    if act == ACT_RELU:
        v = torch.relu(v)
    if mask is not None:
        v = torch.where(mask.double() > 0, v, torch.zeros_like(v))
    return v, bound, _q(bias)


def gemm_tn_ref(g, x):
    """dw = g^T x and the column sums of g."""
    dw = g.double().t() @ x.double()
    bound = g.double().abs().t() @ x.double().abs()
    cs = g.double().sum(0)
    return dw, cs, max(bound.max(), g.double().abs().sum(0).max()).reshape(1), 1.0


def crossnet_ref(x0, xl, W, bias):
    """(out, lin) = (x0 * (xl W^T + b) + xl, xl W^T + b): out from the
    unrounded lin."""
    lin = xl.double() @ W.double().t()
    bound = xl.double().abs() @ W.double().abs().t()
    if bias is not None:
        lin = lin + bias.double()
        bound = bound + bias.double().abs()
    out = x0.double() * lin + xl.double()
    full = torch.maximum(bound, x0.double().abs() * bound + xl.double().abs())
    return out, lin, full, _q(bias)


def crossnet_dx_ref(u, W, g):
    """u W + g (the kernel takes wt = W^T)."""
    v = u.double() @ W.double() + g.double()
    return v, u.double().abs() @ W.double().abs() + g.double().abs(), 1.0


def mlp_head_ref(h, w, bias, gz):
    """z = h w + bias; grad_h = gz w where h > 0; dw = gz^T h; db = sum gz."""
    hd, wd, gd = h.double(), w.double(), gz.double()
    z = hd @ wd
    bound = hd.abs() @ wd.abs()
    if bias is not None:
        z = z + bias.double()
        bound = bound + bias.double().abs()
    gh = torch.where(hd > 0, gd[:, None] * wd[None, :], torch.zeros_like(hd))
    dw = gd @ hd
    db = gd.sum()
    top = max(bound.max(), (gd.abs() @ hd.abs()).max(), gd.abs().sum(),
              (gd.abs()[:, None] * wd.abs()[None, :]).max())
    return z, gh, dw, db, top.reshape(1), _q(bias)


def tril_pairs(F, device):
    i, j = torch.tril_indices(F, F, -1, device=device)
    return i, j


def dot_ref(x):
    """Strictly-lower triangle of X X^T, row-major."""
    xd = x.double()
    i, j = tril_pairs(x.shape[1], x.device)
    z = torch.bmm(xd, xd.transpose(1, 2))
    bound = torch.bmm(xd.abs(), xd.abs().transpose(1, 2))
    return z[:, i, j], bound, 1.0


def dot_grad_ref(x, top_grad):
    """grad_x = S X, S the symmetric completion of top_grad (zero diagonal)."""
    B, F, _ = x.shape
    i, j = tril_pairs(F, x.device)
    S = torch.zeros(B, F, F, dtype=torch.float64, device=x.device)
    S[:, i, j] = top_grad.double()
    S[:, j, i] = top_grad.double()
    return torch.bmm(S, x.double()), torch.bmm(S.abs(), x.double().abs()), 1.0


# ---------------------------------------------------------------------------
# Guarded buffers
# ---------------------------------------------------------------------------
GUARD_ROWS = 8


class Guarded:
    """An output [rows, cols] that is a view of a larger buffer pre-filled
    with SENTINEL: GUARD_ROWS extra rows after the last one and, with
    ld > cols, extra columns.  check() asserts the guard cells still hold
    the sentinel; it only reads the buffer itself."""

    def __init__(self, rows, cols, dtype, device, ld=None):
        self.rows, self.cols = rows, cols
        self.ld = cols if ld is None else ld
        self.buf = torch.full((rows + GUARD_ROWS, self.ld), SENTINEL, dtype=dtype, device=device)
        self.view = self.buf[:rows, :cols]

    def check(self, name="output"):
        bad = self.buf != SENTINEL
        bad[:self.rows, :self.cols] = False
        if bool(bad.any()):
            idx = bad.nonzero()[:8].tolist()
            raise AssertionError("%s: %d guard cells overwritten (rows past %d / columns past %d), "
                                 "first at %s" % (name, int(bad.sum()), self.rows, self.cols, idx))


def nan_padded(t, device, ld=None, col_off=0):
    """t [rows, ..., cols] as the leading rows (and, with ld, a column window
    starting at col_off) of a larger NaN-filled device buffer: rows or
    columns past the end that leak into kept outputs show as NaNs, and a
    kernel that stages whole tiles stays inside the allocation.  The row
    padding reaches the next multiple of 256 rows plus GUARD_ROWS."""
    rows, cols = t.shape[0], t.shape[-1]
    extra = (-rows) % 256 + GUARD_ROWS
    shape = (rows + extra,) + tuple(t.shape[1:-1]) + (cols if ld is None else ld,)
    buf = torch.full(shape, float("nan"), dtype=t.dtype, device=device)
    view = buf[:rows, ..., col_off:col_off + cols]
    view.copy_(t)
    return view


def with_teeth(build, outputs, tries=64):
    """build(seed) -> a case (a tuple); outputs(case) -> the fp32 references
    of its bf16 outputs.  Returns the first case, over seeds 0, 1, ..., whose
    references all pass assert_teeth: with a handful of output elements (one
    row, one logit) a given draw may hold no tie.  The choice looks at the
    reference alone."""
    last = None
    for seed in range(tries):
        case = build(seed)
        try:
            for ref in outputs(case):
                assert_teeth(ref)
            return case
        except AssertionError as e:
            last = e
    raise AssertionError("no seed in %d gives the case teeth: %s" % (tries, last))


# ---------------------------------------------------------------------------
# Comparison and the mismatch report
# ---------------------------------------------------------------------------
def mismatch_report(got, want, name="output", first=6):
    """What whoever fixes a kernel will want: how many elements are wrong,
    the first few (row, col, got, want), and where the wrong elements sit
    relative to the tile edges (row and column indices mod 64 / 128 / 256)."""
    g = got.reshape(got.shape[0], -1) if got.dim() != 2 else got
    w = want.reshape(want.shape[0], -1) if want.dim() != 2 else want
    g, w = g.double(), w.double()
    bad = (g != w) | g.isnan()
    n = int(bad.sum())
    lines = ["%s: %d of %d elements wrong, shape %s" % (name, n, bad.numel(), tuple(got.shape))]
    if n == 0:
        return lines[0]
    idx = bad.nonzero()
    for r, c in idx[:first].tolist():
        lines.append("  (%d, %d): got %r, want %r" % (r, c, float(g[r, c]), float(w[r, c])))
    rows, cols = idx[:, 0], idx[:, 1]
    lines.append("  rows %d..%d (%d distinct), columns %d..%d (%d distinct)"
                 % (int(rows.min()), int(rows.max()), rows.unique().numel(),
                    int(cols.min()), int(cols.max()), cols.unique().numel()))
    for m in (64, 128, 256):
        rm, cm = (rows % m), (cols % m)
        lines.append("  mod %3d: rows in [%d, %d], columns in [%d, %d]; %d on a tile's last row, "
                     "%d on its first, %d on a tile's last column, %d on its first"
                     % (m, int(rm.min()), int(rm.max()), int(cm.min()), int(cm.max()),
                        int((rm == m - 1).sum()), int((rm == 0).sum()),
                        int((cm == m - 1).sum()), int((cm == 0).sum())))
    return "\n".join(lines)


def assert_equal(got, want, name="output"):
    """No NaNs, same dtype and shape, and torch.equal (values: -0 == +0)."""
    assert got.dtype == want.dtype and got.shape == want.shape, \
        (name, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if bool(got.isnan().any()) or not torch.equal(got, want):
        raise AssertionError(mismatch_report(got, want, name))


# ---------------------------------------------------------------------------
# Deliberate mutations of a reference (tests/test_gemm_exact_reference.py):
# what a subtly wrong kernel would compute
# ---------------------------------------------------------------------------
def bf16_truncate(x32):
    """fp32 -> bf16 by dropping the low 16 bits."""
    bits = x32.float().contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).to(torch.bfloat16)


# ---------------------------------------------------------------------------
# Runners: the C entries on guarded buffers (GPU)
# ---------------------------------------------------------------------------
def _abi():
    from deeprec_amd import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_handle


def run_crossnet_forward(x0, xl, W, bias, with_lin, device, entry="forward", bias_offset=0):
    """dr_crossnet_forward_bf16 (entry "layer": dr_crossnet_layer_bf16) on
    NaN-padded inputs and sentinel-guarded outputs -> (out, lin or None)
    after the guards were checked.  bias_offset: bias starts that many floats
    into its buffer (1: 4-B aligned only)."""
    lib, check, ptr, stream = _abi()
    B, d = x0.shape
    a0, al = nan_padded(x0, device), nan_padded(xl, device)
    w = W.to(device).contiguous()
    b = None
    if bias is not None:
        bbuf = torch.full((d + bias_offset + 4,), float("nan"), dtype=torch.float32, device=device)
        b = bbuf[bias_offset:bias_offset + d]
        b.copy_(bias)
    out = Guarded(B, d, torch.bfloat16, device)
    lin = Guarded(B, d, torch.bfloat16, device) if with_lin else None
    if entry == "layer":
        assert not with_lin
        check(lib.dr_crossnet_layer_bf16(ptr(a0), ptr(al), ptr(w), ptr(b), B, d, ptr(out.view),
                                         stream(device)))
    else:
        check(lib.dr_crossnet_forward_bf16(ptr(a0), ptr(al), ptr(w), ptr(b), B, d, ptr(out.view),
                                           ptr(lin.view) if lin else None, stream(device)))
    torch.cuda.synchronize(device)
    out.check("out")
    if lin:
        lin.check("lin")
    return out.view, (lin.view if lin else None)


def run_crossnet_dx(u, wt, g, device):
    lib, check, ptr, stream = _abi()
    B, d = u.shape
    uu, gg = nan_padded(u, device), nan_padded(g, device)
    w = wt.to(device).contiguous()
    dx = Guarded(B, d, torch.bfloat16, device)
    check(lib.dr_crossnet_dx_bf16(ptr(uu), ptr(w), ptr(gg), B, d, ptr(dx.view), stream(device)))
    torch.cuda.synchronize(device)
    dx.check("dx")
    return dx.view


# ---------------------------------------------------------------------------
# CrossNet cases shared by the GPU test and the child process
# ---------------------------------------------------------------------------
def crossnet_range(d, bias):
    """Operand range r (xl and W in [-r, r]; x0 in [-4, 4]) for width d.
    Integers up to 256 are bf16 numbers, so without a fractional bias the
    outputs must pass 256 to be inexact: lin has a standard deviation of
    about sqrt(d) r (r + 1) / 3, aimed at a few hundred (bf16 steps of 2 to
    8, where one integer in 2 to 8 is a tie).  With a bias in multiples of
    0.25 the plain range 4 has teeth from d = 256 (14 to 19 % ties)."""
    if d >= 256 and bias:
        return 4
    for r in range(4, 33):
        if d ** 0.5 * r * (r + 1) / 3.0 >= 450.0:
            return r
    return 32


def crossnet_case(B, d, bias, device, need_teeth=True):
    """One forward case: inputs (CPU), fp32-exact references of out and lin
    (on device), after assert_exact_inputs and assert_teeth on both."""
    r = crossnet_range(d, bias)

    def build(seed):
        g = gen(1000 * B + d + (7 if bias else 0) + 100003 * seed)
        x0, xl, W = ints(g, (B, d), 4), ints(g, (B, d), r), ints(g, (d, d), r)
        b = quarters(g, d, 4) if bias else None
        dev = [t.to(device) for t in (x0, xl, W)] + [b.to(device) if bias else None]
        out, lin, bound, q = crossnet_ref(*dev)
        assert_exact_inputs(bound, q, bf16=dev[:3], multiples=[(t, 1.0) for t in dev[:3]] +
                            ([(dev[3], 0.25)] if bias else []))
        return (x0, xl, W, b), to_f32(out), to_f32(lin)

    return with_teeth(build, lambda c: c[1:]) if need_teeth else build(0)


def crossnet_dx_case(B, d, device):
    r = crossnet_range(d, False)

    def build(seed):
        g = gen(77 + 1000 * B + d + 100003 * seed)
        u, W, gg = ints(g, (B, d), r), ints(g, (d, d), r), ints(g, (B, d), 4)
        dev = [t.to(device) for t in (u, W, gg)]
        v, bound, q = crossnet_dx_ref(*dev)
        assert_exact_inputs(bound, q, bf16=dev, multiples=[(t, 1.0) for t in dev])
        return (u, W, gg), to_f32(v)

    return with_teeth(build, lambda c: c[1:])


def check_crossnet_forward(case, with_lin, device, entry="forward", bias_offset=0, name=""):
    (x0, xl, W, b), want_out, want_lin = case
    out, lin = run_crossnet_forward(x0, xl, W, b, with_lin, device, entry, bias_offset)
    assert_equal(out, want_out.to(torch.bfloat16), "crossnet out " + name)
    if with_lin:
        assert_equal(lin, want_lin.to(torch.bfloat16), "crossnet lin " + name)


def check_crossnet_dx(case, device, name=""):
    (u, W, g), want = case
    dx = run_crossnet_dx(u, W.t().contiguous(), g, device)
    assert_equal(dx, want.to(torch.bfloat16), "crossnet dx " + name)


# ---------------------------------------------------------------------------
# Child process: python tests/gemm_exact.py crossnet
# ---------------------------------------------------------------------------
def _child_crossnet():
    """The forward cases (257, 320) and (513, 64) and the dx case (257, 320)
    under whatever DR_CROSSNET_VARIANT / DR_CROSSNET_LEGACY this process was
    started with (the library reads them once).  The legacy path has no
    lin_out.  Prints each mismatch report; returns the exit status."""
    device = "cuda:0"
    legacy = os.environ.get("DR_CROSSNET_LEGACY") is not None
    failed = 0
    if legacy:
        # the variable reached the library: the legacy path refuses lin_out
        # (an argument check, before any launch)
        from deeprec_amd._lib import InvalidArgumentError
        try:
            check_crossnet_forward(crossnet_case(1, 64, True, device), True, device)
            failed += 1
            print("MISMATCH: DR_CROSSNET_LEGACY is set but lin_out was accepted", flush=True)
        except InvalidArgumentError:
            print("ok: the legacy path refuses lin_out", flush=True)
    jobs = [("forward", 257, 320), ("forward", 513, 64), ("dx", 257, 320)]
    for kind, B, d in jobs:
        try:
            name = "(B=%d, d=%d)" % (B, d)
            if kind == "forward":
                check_crossnet_forward(crossnet_case(B, d, True, device), not legacy, device,
                                       name=name)
            else:
                check_crossnet_dx(crossnet_dx_case(B, d, device), device, name=name)
            print("ok: %s (%d, %d)" % (kind, B, d), flush=True)
        except AssertionError as e:
            failed += 1
            print("MISMATCH: %s (%d, %d)\n%s" % (kind, B, d, e), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    # the paths tests/conftest.py sets, for a process pytest did not start
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "deeprec-1_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    if sys.argv[1:] != ["crossnet"]:
        sys.exit("usage: python tests/gemm_exact.py crossnet")
    sys.exit(_child_crossnet())
