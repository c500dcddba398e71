"""The co-action kernels (csrc/co_action.hip) against the fp64 composition
of co_action_ref.py, and their exactness properties.  Bound: rtol = atol = 1e-5 of fp64 (the
project's kernel bound); the fp32 torch twin on the CPU reaches 0.060 of it at worst on these
seeds (out of the maximum shape) and is exact on the integer operands."""
import pytest
import torch

import co_action_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(key, rows=slice(None)):
    cs = ref.case(key, "real")
    return [cs[n][rows].float().to(DEV).contiguous() for n in ("param", "his", "mask", "go")]


def _kernels(key, rows=slice(None), t=None):
    """(out, grad_his, grad_param) of the raw entries."""
    from deeprec_amd import ops
    param, his, mask, go = t or _inputs(key, rows)
    assert ops._CO_ACTION_NATIVE and ops.co_action_native_ok(param, his, mask, key[2], key[3])
    out = ops.co_action_forward(param, his, mask, *key[2:])
    return (out,) + ops.co_action_backward(param, his, mask, go, *key[2:])


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert torch.equal(x, y)


@pytest.mark.parametrize("key", ref.CASES)
def test_real_operands_are_within_the_bound(key):
    from deeprec_amd import ops
    want = ref.reference(key, "real")
    got = ref.run(key, ref.case(key, "real"), ops.co_action, torch.float32, DEV)
    errs = {n: ref.ratio(got[n], want[n]) for n in ref.NAMES}
    print("co_action %s: error / bound: %s" % (key, ", ".join("%s %.3f" % e for e in errs.items())))
    assert max(errs.values()) <= 1.0, errs


@pytest.mark.parametrize("key", ref.INTEGER_CASES)
def test_integer_operands_are_reproduced_exactly(key):
    from deeprec_amd import ops
    want = ref.reference(key, "integer")
    got = ref.run(key, ref.case(key, "integer"), ops.co_action, torch.float32, DEV)
    for n in ref.NAMES:
        assert torch.equal(got[n].cpu(), want[n].float()), n


@pytest.mark.parametrize("key", ref.CASES)
def test_a_sample_does_not_depend_on_its_batch_and_masked_places_are_zero(key):
    B, mask = key[0], ref.case(key, "real")["mask"]
    full = _kernels(key)
    for b in sorted({0, B // 2, B - 1}):
        _same(_kernels(key, rows=slice(b, b + 1)), [x[b:b + 1] for x in full])
    _same(_kernels(key), full)
    assert not full[1][(mask == 0).to(DEV)].any()
    if B > 1:                                               # the last sample is all masked
        assert not full[0][-1].any() and not full[2][-1].any()


@pytest.mark.parametrize("key", [ref.CASES[2], ref.CASES[3]])
def test_column_blocks_are_read_in_place(key):
    param, his, mask, go = _inputs(key)
    x = torch.cat([torch.full_like(his, float("nan")), his], -1)
    w = torch.cat([torch.full_like(param, float("nan")), param], -1)
    xs, ws = x[..., his.shape[2]:], w[:, param.shape[1]:]
    assert not xs.is_contiguous() and not ws.is_contiguous()
    _same(_kernels(key, t=(ws, xs, mask, go)), _kernels(key, t=(param, his, mask, go)))


@pytest.mark.parametrize("key", [ref.CASES[2], ref.CASES[3]])
def test_forward_and_backward_capture_on_one_stream(key):
    t = _inputs(key)
    eager = _kernels(key, t=t)                              # warm-up, and the result to match
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # one stream, no parallel branches
        captured = _kernels(key, t=t)
    for i in range(3):                                      # several replays, each from NaNs
        [x.fill_(float("nan")) for x in captured]
        g.replay()
        torch.cuda.synchronize()
        _same(captured, eager)


@pytest.mark.parametrize("how", ["width 36", "DR_CO_ACTION=torch"])
def test_the_torch_composition_serves_what_the_kernels_do_not(how, monkeypatch):
    from deeprec_amd import ops
    key = (3, 5, (36, 8, 4), 2, True, False) if how == "width 36" else ref.CASES[2]
    cs, want = ref.case(key, "real"), ref.reference(key, "real")
    if how == "width 36":
        param, his, mask = [cs[n].float().to(DEV) for n in ("param", "his", "mask")]
        assert not ops.co_action_native_ok(param, his, mask, key[2], key[3])
        with pytest.raises(Exception, match="co_action"):   # the kernels themselves refuse
            ops.co_action_forward(param, his, mask, *key[2:])
    else:
        monkeypatch.setattr(ops, "_CO_ACTION_NATIVE", False)    # what the variable sets at import

    def no_kernel(*a, **k):
        raise AssertionError("the native path ran")
    monkeypatch.setattr(ops, "co_action_forward", no_kernel)
    got = ref.run(key, cs, ops.co_action, torch.float32, DEV)
    for n in ref.NAMES:
        assert ref.ratio(got[n], want[n]) <= 1.0, n
