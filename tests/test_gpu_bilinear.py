"""The bilinear-interaction kernels (csrc/bilinear.hip) against the fp64
composition of bilinear_ref.py, and their exactness properties.  Bound: rtol = atol = 1e-5 of
fp64 (the project's kernel bound); the fp32 torch composition on the CPU stays at or below 0.37
of it on these inputs (grad_W, kind all, at (2, 64, 64)) and is exact on the integer operands."""
import pytest
import torch

import bilinear_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(cs, rows=slice(None)):
    """fp32 device tensors of a case (x, w, scale, go)."""
    t = {n: None if cs[n] is None else cs[n].float().to(DEV) for n in cs}
    scale = None if t["scale"] is None else t["scale"][rows].contiguous()
    return t["x"][rows].contiguous(), t["w"], scale, t["go"][rows].contiguous()


def _kernels(cs, kind, rows=slice(None), t=None):
    """(out, grad_x, grad_scale, grad_W) of the raw entries."""
    from deeprec_amd import ops
    x, w, scale, go = t or _inputs(cs, rows)
    assert ops._BILINEAR_NATIVE and ops.bilinear_native_ok(x, w, scale)
    out = ops.bilinear_forward(x, w, kind, scale)
    gx, gs, gw = ops.bilinear_backward(x, w, kind, go, scale)
    return out, gx, gs, gw


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("case", ref.CASES)
def test_integer_operands_are_reproduced_exactly(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case, "integer"), ref.reference(*case, "integer")
    got = ref.run(cs, case[1], ops.bilinear_interaction, torch.float32, DEV)
    for n in ref.NAMES:
        assert (got[n] is None and want[n] is None) or torch.equal(got[n].cpu().double(), want[n]), n
    _same(_kernels(cs, case[1]), [got[n] for n in ref.NAMES])


@pytest.mark.parametrize("case", ref.CASES)
def test_real_operands_are_within_the_bound(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case, "real"), ref.reference(*case, "real")
    got = ref.run(cs, case[1], ops.bilinear_interaction, torch.float32, DEV)
    errs = {n: ref.ratio(got[n], want[n]) for n in ref.NAMES if want[n] is not None}
    print("bilinear %s: error / bound: %s" % (case, ", ".join("%s %.3f" % e for e in errs.items())))
    assert max(errs.values()) <= 1.0, errs


@pytest.mark.parametrize("case", ref.CASES)
def test_a_sample_does_not_depend_on_its_batch_and_runs_repeat(case):
    B, cs = case[0][0], ref.case(*case, "real")
    full = _kernels(cs, case[1])
    for b in sorted({0, B // 2, B - 1}):
        _same(_kernels(cs, case[1], rows=slice(b, b + 1))[:3], [x if x is None else x[b:b + 1]
                                                                for x in full[:3]])
    _same(_kernels(cs, case[1]), full)


@pytest.mark.parametrize("case", [(ref.SHAPES[2], "each", True), (ref.SHAPES[3], "interaction",
                                                                  False)])
def test_forward_and_backward_capture_on_one_stream(case):
    t = _inputs(ref.case(*case, "real"))
    eager = _kernels(None, case[1], t=t)                    # warm-up, and the result to match
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # one stream, no parallel branches
        captured = _kernels(None, case[1], t=t)
    for i in range(3):                                      # several replays, each from NaNs
        [x.fill_(float("nan")) for x in captured if x is not None]
        g.replay()
        torch.cuda.synchronize()
        _same(captured, eager)


@pytest.mark.parametrize("how", ["width 65", "DR_BILINEAR=torch"])
def test_the_torch_composition_serves_what_the_kernels_do_not(how, monkeypatch):
    from deeprec_amd import ops
    key = ((3, 5, 65) if how == "width 65" else ref.SHAPES[1], "each", True, "real")
    cs, want = ref.case(*key), ref.reference(*key)
    if how == "width 65":
        x, w = cs["x"].float().to(DEV), cs["w"].float().to(DEV)
        assert not ops.bilinear_native_ok(x, w)
        with pytest.raises(Exception, match="bilinear"):    # the kernels themselves refuse
            ops.bilinear_forward(x, w, "each")
    else:
        monkeypatch.setattr(ops, "_BILINEAR_NATIVE", False)  # what DR_BILINEAR=torch sets at import

    def no_kernel(*a, **k):
        raise AssertionError("the native path ran")
    monkeypatch.setattr(ops, "bilinear_forward", no_kernel)
    got = ref.run(cs, "each", ops.bilinear_interaction, torch.float32, DEV)
    for n in ref.NAMES:
        assert ref.ratio(got[n], want[n]) <= 1.0, n
