"""The CIN kernels (csrc/cin.hip) against the fp64 composition of
cin_ref.py, and their exactness properties.  Bound: rtol = atol = 1e-5 of fp64 (the project's
kernel bound); the fp32 torch twin on the CPU reaches 0.19 of it at worst (grad_W of the
hidden-layer shape) and is exact on the integer operands."""
import pytest
import torch

import cin_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(cs, rows=slice(None)):
    """fp32 device tensors of a case (x0, xk, w, bias, go); xk None: x0 twice."""
    t = {n: None if cs[n] is None else cs[n].float().to(DEV) for n in cs}
    x0 = t["x0"][rows].contiguous()
    xk = x0 if t["xk"] is None else t["xk"][rows].contiguous()
    return x0, xk, t["w"], t["bias"], t["go"][rows].contiguous()


def _kernels(cs, rows=slice(None), t=None):
    """(out, grad_x0, grad_xk, grad_W, grad_bias) of the raw entries."""
    from deeprec_amd import ops
    x0, xk, w, bias, go = t or _inputs(cs, rows)
    assert ops._CIN_NATIVE and ops.cin_native_ok(x0, xk, w)
    out = ops.cin_forward(x0, xk, w, bias)
    gxk, gx0, gw, gb = ops.cin_backward(x0, xk, w, go, bias is not None)
    return out, gx0, gxk, gw, gb


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("case", ref.CASES)
def test_integer_operands_are_reproduced_exactly(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case, "integer"), ref.reference(*case, "integer")
    got = ref.run(cs, ops.cin_layer, torch.float32, DEV)
    for n in ref.NAMES:
        assert (got[n] is None and want[n] is None) or torch.equal(got[n].cpu(), want[n].float()), n
    out, gx0, gxk, gw, gb = _kernels(cs)
    if cs["xk"] is None:
        gx0, gxk = gx0 + gxk, None
    _same((out, gx0, gxk, gw, gb), [got[n] for n in ref.NAMES])


@pytest.mark.parametrize("case", ref.CASES)
def test_real_operands_are_within_the_bound(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case, "real"), ref.reference(*case, "real")
    got = ref.run(cs, ops.cin_layer, torch.float32, DEV)
    errs = {n: ref.ratio(got[n], want[n]) for n in ref.NAMES if want[n] is not None}
    print("cin %s: error / bound: %s" % (case, ", ".join("%s %.3f" % e for e in errs.items())))
    assert max(errs.values()) <= 1.0, errs


@pytest.mark.parametrize("case", ref.CASES)
def test_a_sample_does_not_depend_on_its_batch_and_runs_repeat(case):
    B, cs = case[0][0], ref.case(*case, "real")
    full = _kernels(cs)
    for b in sorted({0, B // 2, B - 1}):
        _same(_kernels(cs, rows=slice(b, b + 1))[:3], [x[b:b + 1] for x in full[:3]])
    _same(_kernels(cs), full)


@pytest.mark.parametrize("case", [(ref.SHAPES[1], True, True), (ref.SHAPES[3], True, False)])
def test_forward_and_backward_capture_on_one_stream(case):
    t = _inputs(ref.case(*case, "real"))
    eager = _kernels(None, t=t)                             # warm-up, and the result to match
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # one stream, no parallel branches
        captured = _kernels(None, t=t)
    for i in range(3):                                      # several replays, each from NaNs
        [x.fill_(float("nan")) for x in captured]
        g.replay()
        torch.cuda.synchronize()
        _same(captured, eager)


@pytest.mark.parametrize("how", ["width 65", "DR_CIN=torch"])
def test_the_torch_composition_serves_what_the_kernels_do_not(how, monkeypatch):
    from deeprec_amd import ops
    key = ((3, 5, 5, 6, 65) if how == "width 65" else ref.SHAPES[1], True, False, "real")
    cs, want = ref.case(*key), ref.reference(*key)
    if how == "width 65":
        x = cs["x0"].float().to(DEV)
        assert not ops.cin_native_ok(x, cs["xk"].float().to(DEV), cs["w"].float().to(DEV))
        with pytest.raises(Exception, match="cin"):         # the kernels themselves refuse
            ops.cin_forward(x, cs["xk"].float().to(DEV), cs["w"].float().to(DEV))
    else:
        monkeypatch.setattr(ops, "_CIN_NATIVE", False)      # what DR_CIN=torch sets at import

    def no_kernel(*a, **k):
        raise AssertionError("the native path ran")
    monkeypatch.setattr(ops, "cin_forward", no_kernel)
    got = ref.run(cs, ops.cin_layer, torch.float32, DEV)
    for n in ref.NAMES:
        assert ref.ratio(got[n], want[n]) <= 1.0, n
