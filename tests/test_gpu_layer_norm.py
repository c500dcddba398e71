"""The layer-norm / relu / mask-multiply kernels (csrc/layer_norm.hip)
against the fp64 composition of layer_norm_ref.py, and their exactness properties.
Bound: rtol = atol = 1e-5 of fp64 (the project's kernel bound); an fp32 torch twin of the
first seven shapes reaches 0.55 of it at worst (dgain)."""
import pytest
import torch

import layer_norm_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, D, P): every minimum; BST's width, 4 rows per wave, odd B; 9 chunks in a 16-lane
# group; 16 rows per wave and a ragged last block; two chunks per lane, the second ragged;
# every maximum; many block partials for the finishing kernel (this one without residual and
# mask); more tiles than the persistent backward grid has blocks (1024 of 64 rows)
SHAPES = [(3, 4, 1), (5, 64, 1), (2, 36, 3), (70, 16, 2), (3, 416, 2), (2, 1024, 8),
          (600, 128, 1), (65606, 16, 1)]
CASES = [s + (relu, 1e-3 if (i + relu) % 2 else 1e-8, s[0] == 600)
         for i, s in enumerate(SHAPES) for relu in (False, True)]
T = ("x", "gain", "bias", "residual", "mask", "go")


def _inputs(cs, rows=slice(None), views=False):
    """fp32 device tensors of a case; views: x, residual, mask and go as column blocks of
    wider NaN-filled buffers."""
    t = {n: None if cs[n] is None else cs[n].float().to(DEV) for n in T}
    for n in ("x", "residual", "mask", "go"):
        if t[n] is None:
            continue
        t[n] = t[n][rows].contiguous()
        if views:
            l, w = {"x": (4, 8), "residual": (8, 4), "mask": (0, 12), "go": (12, 0)}[n], t[n][0].numel()
            p = torch.nn.functional.pad(t[n].flatten(1), l, value=float("nan"))
            t[n] = p[:, l[0]:l[0] + w].view(t[n].shape)
            assert not t[n].is_contiguous() or t[n].shape[0] == 1
    return t


def _kernels(t, cs):                    # (out, saved, dx, dmask, dgain, dbias) of the raw entries
    from deeprec_amd import ops
    out, saved = ops.layer_norm_forward(t["x"], t["gain"], t["bias"], cs["eps"], t["residual"],
                                        t["mask"], cs["relu"])
    return (out, saved) + ops.layer_norm_backward(t["x"], t["gain"], t["bias"], saved, t["go"],
                                                  t["residual"], t["mask"], cs["relu"])


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("case", CASES)
def test_values_match_fp64_from_contiguous_inputs_and_views(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case), ref.reference(*case)
    t = _inputs(cs)
    assert ops._LAYER_NORM_NATIVE
    assert ops.layer_norm_native_ok(t["x"], t["gain"], t["bias"], t["residual"], t["mask"])
    got = ref.run(cs, ops.layer_norm, torch.float32, DEV)
    errs = {n: ref.ratio(got[n], want[n]) for n in got}
    print("layer_norm %s: error / bound: %s" % (case, ", ".join("%s %.3f" % e for e in errs.items())))
    assert max(errs.values()) <= 1.0, errs
    out, _, dx, dmask, dgain, dbias = plain = _kernels(t, cs)
    _same((out, dx, dmask, dgain, dbias), [got.get(n) for n in ref.NAMES])
    _same(_kernels(_inputs(cs, views=True), cs), plain)


@pytest.mark.parametrize("case", CASES)
def test_a_row_does_not_depend_on_its_batch_and_runs_repeat(case):
    B, cs = case[0], ref.case(*case)
    out, saved, dx, dmask, dgain, dbias = full = _kernels(_inputs(cs), cs)
    for b in sorted({0, B // 2, B - 1}):
        alone = _kernels(_inputs(cs, rows=slice(b, b + 1)), cs)
        _same(alone[:4], [None if x is None else x[b:b + 1] for x in full[:4]])
    _same(_kernels(_inputs(cs), cs), full)


@pytest.mark.parametrize("case", CASES)
def test_forward_and_backward_capture_on_one_stream(case):
    cs = ref.case(*case)
    t = _inputs(cs, views=True)
    eager = _kernels(t, cs)                                 # warm-up, and the result to match
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # one stream, no parallel branches
        captured = _kernels(t, cs)
    for i in range(3):                                      # several replays, each from NaNs
        [x.fill_(float("nan")) for x in captured if x is not None]
        g.replay()
        torch.cuda.synchronize()
        _same(captured, eager)


@pytest.mark.parametrize("case", [(3, 6, 2, True, 1e-3, False), (2, 8, 9, False, 1e-8, False)])
def test_shapes_outside_the_native_set_take_the_torch_composition(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case), ref.reference(*case)
    t = _inputs(cs)
    assert not ops.layer_norm_native_ok(t["x"], t["gain"], t["bias"], t["residual"], t["mask"])
    got = ref.run(cs, ops.layer_norm, torch.float32, DEV)
    for n in got:
        assert ref.ratio(got[n], want[n]) <= 1.0, n
    with pytest.raises(Exception, match="layer_norm"):      # the kernels themselves refuse
        _kernels(t, cs)
