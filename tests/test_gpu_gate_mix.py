"""The gate softmax / expert mixing kernels (csrc/gate_mix.hip)
against the fp64 composition of gate_mix_ref.py, and their exactness properties.
Bound: rtol = atol = 1e-5 of fp64 (the project's kernel bound); an fp32 torch twin
of this case set reaches 0.19 of it (grad_logits at H = 512), 0.07 elsewhere."""
import pytest
import torch

import gate_mix_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, K, E, H): the MMoE shape, two samples per wave and an odd B; H / 4 = 9 with odd K
# and E; every minimum; 16 samples per wave and a ragged last block (tile 64); every
# maximum, K E = 128; two chunks per lane, the second partial
SHAPES = [(5, 2, 8, 128), (3, 3, 5, 36), (2, 1, 1, 4), (70, 2, 4, 16), (3, 8, 16, 512),
          (4, 4, 6, 260)]
CASES = [s + (ple,) for s in SHAPES for ple in (False, True)]


def _inputs(cs, rows=slice(None), views=False):
    """fp32 device z, h, go of a case; views: column blocks of wider buffers (z, h) and a
    row stride (go)."""
    z, h, go = (cs[n][rows].float().contiguous().to(DEV) for n in ("z", "h", "go"))
    if views:
        def wide(x, l, r):              # NaNs around the block; the row stride a multiple of 4
            r += -(x[0].numel() + l + r) % 4
            p = torch.nn.functional.pad(x.flatten(1), (l, r), value=float("nan"))
            return p[:, l:l + x[0].numel()].view(x.shape)
        z, h, go = wide(z, 4, 8), wide(h, 8, 4), wide(go, 0, 12)
        assert not (z.is_contiguous() or h.is_contiguous() or go.is_contiguous())
    return z, h, go


def _kernels(z, h, go, select):         # (out, gates, grad_logits, grad_experts) of the two kernels
    from deeprec_amd import ops
    out, gates = ops.gate_mix_forward(z, h, select)
    return (out, gates) + ops.gate_mix_backward(h, gates, go, select)


def _native(cs, **kw):
    return _kernels(*_inputs(cs, **kw), cs["select"])


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case", CASES)
def test_values_match_fp64_from_contiguous_inputs_and_views(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case), ref.reference(*case)
    assert ops._GATE_MIX_NATIVE and ops.gate_mix_native_ok(*_inputs(cs)[:2])
    got = ref.run(cs, ops.gate_mix, torch.float32, DEV)
    plain = _native(cs)
    got["gates"] = plain[1]
    errs = {n: ref.ratio(got[n], want[n]) for n in ref.NAMES}
    print("gate_mix %s: error / bound: %s" % (case, ", ".join("%s %.3f" % e for e in errs.items())))
    assert max(errs.values()) <= 1.0, errs
    _same(plain, [got[n] for n in ref.NAMES])
    _same(_native(cs, views=True), plain)


@pytest.mark.parametrize("case", CASES)
def test_unselected_entries_are_exact_zeros_and_runs_repeat(case):
    B, K, E, H, ple = case
    cs = ref.case(*case)
    out, gates, gz, gh = res = _native(cs)
    sel = torch.ones(K, E, dtype=torch.bool) if cs["select"] is None else cs["select"]
    for t in res:
        assert torch.isfinite(t).all()
    off, one = ~sel.to(DEV), (sel.sum(1) == 1).to(DEV)
    assert bool(one.any()) == (ple or E == 1)
    for t in (gates, gz):
        assert torch.equal(t[:, off], torch.zeros_like(t[:, off]))
    assert torch.equal(gates[:, one][:, sel.to(DEV)[one]], torch.ones(B, int(one.sum()), device=DEV))
    assert torch.equal(gz[:, one], torch.zeros_like(gz[:, one]))
    assert float(gh.abs().max()) > 0 and (one.all() or float(gz.abs().max()) > 0)
    _same(_native(cs), res)


@pytest.mark.parametrize("case", CASES)
def test_a_sample_does_not_depend_on_its_batch(case):
    B, cs = case[0], ref.case(*case)
    full = _native(cs)
    for b in sorted({0, B // 2, B - 1}):
        _same(_native(cs, rows=slice(b, b + 1)), [x[b:b + 1] for x in full])


@pytest.mark.parametrize("case", CASES)
def test_forward_and_backward_capture_on_one_stream(case):
    cs = ref.case(*case)
    a = _inputs(cs, views=True)
    eager = _kernels(*a, cs["select"])                      # warm-up, and the result to match
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # one stream, no parallel branches
        captured = _kernels(*a, cs["select"])
    for i in range(3):                                      # several replays, each from NaNs
        [t.fill_(float("nan")) for t in captured]
        g.replay()
        torch.cuda.synchronize()
        _same(captured, eager)


@pytest.mark.parametrize("case", [(3, 2, 17, 8, False), (2, 2, 4, 6, True)])
def test_shapes_outside_the_native_set_take_the_torch_composition(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case), ref.reference(*case)
    z, h, _ = _inputs(cs)
    assert not ops.gate_mix_native_ok(z, h)
    got = ref.run(cs, ops.gate_mix, torch.float32, DEV)
    for n in got:
        assert ref.ratio(got[n], want[n]) <= 1.0, n
    with pytest.raises(Exception, match="gate_mix"):        # the kernels themselves refuse
        ops.gate_mix_forward(z, h, cs["select"])
