"""The multi-head self-attention kernels (csrc/mha.hip)
against the fp64 loop reference of mha_ref.py, and their exactness properties.
Bound: rtol = atol = 1e-5 of fp64 (the project's kernel bound); values are of
order 1, sums have at most 128 terms, an fp32 torch twin reaches 0.021 of it."""
import pytest
import torch

import mha_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, T, heads, head_dim): the BST length; the longest T and widest head; one
# key past a tile with an odd head count; exactly one tile; T = 1; a lone sample
SHAPES = [(5, 101, 4, 16), (3, 128, 2, 32), (4, 17, 3, 8), (3, 16, 1, 16), (2, 1, 4, 8),
          (1, 33, 8, 8)]


def _inputs(shape, rows=None, pad=0, cols=None, packed=False):
    """fp32 device inputs of a case: rows picks samples, pad appends random steps, cols picks
    whole heads (views), packed makes q, k, v the column blocks of one [B, T, 3E] tensor."""
    cs = mha_ref.case(*shape)
    q, k, v, go = (cs[n].float() for n in ("q", "k", "v", "go"))
    lens = cs["lens"]
    if pad:
        g = torch.Generator().manual_seed(pad)
        q, k, v, go = (torch.cat([t, torch.randn(t.shape[0], pad, t.shape[2], generator=g)], 1)
                       for t in (q, k, v, go))
    if rows is not None:
        q, k, v, go, lens = (t[rows] for t in (q, k, v, go, lens))
    q, k, v, go, lens = (t.contiguous().to(DEV) for t in (q, k, v, go, lens))
    if cols is not None:                                    # views: the row stride stays E
        q, k, v, go = (t[..., cols] for t in (q, k, v, go))
    if packed:
        E = q.shape[2]
        p = torch.cat([q, k, v], 2)
        q, k, v = p[..., :E], p[..., E:2 * E], p[..., 2 * E:]
    return dict(q=q, k=k, v=v, go=go, lens=lens)


def _native(a, heads):                  # (out, saved, grad_q, grad_k, grad_v) of the two kernels
    from deeprec_amd import ops
    out, saved = ops.mha_seq_forward(a["q"], a["k"], a["v"], a["lens"], heads)
    return (out, saved) + ops.mha_seq_backward(a["q"], a["k"], a["v"], a["lens"], heads, out,
                                               saved, a["go"])


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert torch.equal(x, y)


@pytest.mark.parametrize("shape", SHAPES)
def test_values_match_fp64_from_contiguous_and_packed_inputs(shape):
    from deeprec_amd import ops
    heads, ref, a = shape[2], mha_ref.reference(*shape), _inputs(shape)
    assert ops._MHA_NATIVE and ops.mha_native_ok(a["q"], heads)
    got = mha_ref.run(mha_ref.case(*shape), ops.multihead_attention, torch.float32, DEV)
    errs = {n: mha_ref.ratio(got[n], ref[n]) for n in mha_ref.NAMES}
    print("mha %s: error / bound: %s" % (shape, ", ".join("%s %.3f" % e for e in errs.items())))
    assert max(errs.values()) <= 1.0, errs
    plain, packed = _native(a, heads), _native(_inputs(shape, packed=True), heads)
    assert packed[2].stride(1) == 3 * shape[2] * shape[3]       # one packed gradient buffer
    _same(packed, plain)
    _same((plain[0],) + plain[2:], [got[n] for n in mha_ref.NAMES])


@pytest.mark.parametrize("shape", SHAPES)
def test_padded_positions_are_exact_zeros_and_runs_repeat(shape):
    B, T, heads, _ = shape
    a = _inputs(shape)
    out, saved, gq, gk, gv = res = _native(a, heads)
    pad = torch.arange(T, device=DEV)[None, :] >= a["lens"][:, None]
    assert int(a["lens"][0]) == T and (B == 1 or int(a["lens"][1]) == 0)
    for t in (out, gq, gk, gv):
        assert torch.isfinite(t).all()
        assert torch.equal(t[pad], torch.zeros_like(t[pad]))
    sp = saved.transpose(1, 2)[pad]
    assert torch.isfinite(saved).all() and torch.equal(sp, torch.zeros_like(sp))
    for t in (gq, gk, gv):
        assert float(t[~pad].abs().max()) > 0
    _same(_native(a, heads), res)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_sample_and_a_head_do_not_depend_on_what_surrounds_them(shape):
    B, T, heads, hd = shape
    full = _native(_inputs(shape), heads)
    if T + 9 <= 128:                # 9 more padded steps (past T = 128 there is no kernel)
        longer = _native(_inputs(shape, pad=9), heads)
        _same([longer[1][..., :T]] + [longer[i][:, :T] for i in (0, 2, 3, 4)],
              [full[i] for i in (1, 0, 2, 3, 4)])
    for b in sorted({0, B // 2, B - 1}):
        one = _native(_inputs(shape, rows=slice(b, b + 1)), heads)
        _same(one, [x[b:b + 1] for x in full])
    if heads >= 2:                                           # heads h, h + 1 as the only heads
        h = heads // 2 - 1 if heads > 2 else 0
        cols = slice(h * hd, (h + 2) * hd)
        two = _native(_inputs(shape, cols=cols), 2)
        _same(two, [full[0][..., cols], full[1][:, h:h + 2]] + [x[..., cols] for x in full[2:]])


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_backward_capture_on_one_stream(shape):
    a = _inputs(shape, packed=True)
    eager = _native(a, shape[2])                            # warm-up, and the result to match
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # one stream, no parallel branches
        captured = _native(a, shape[2])
    for i in range(3):                                      # several replays, each from NaNs
        [t.fill_(float("nan")) for t in (captured[0], captured[1], captured[2]._base)]
        g.replay()
        torch.cuda.synchronize()
        _same(captured, eager)


@pytest.mark.parametrize("B,T,heads,hd", [(3, 9, 2, 12), (2, 130, 2, 16)])
def test_shapes_outside_the_native_set_take_the_torch_composition(B, T, heads, hd):
    from deeprec_amd import ops
    cs, ref = mha_ref.case(B, T, heads, hd), mha_ref.reference(B, T, heads, hd)
    assert not ops.mha_native_ok(cs["q"].float().to(DEV), heads)
    got = mha_ref.run(cs, ops.multihead_attention, torch.float32, DEV)
    for n in mha_ref.NAMES:
        assert mha_ref.ratio(got[n], ref[n]) <= 1.0, n
    a = _inputs((B, T, heads, hd))
    with pytest.raises(Exception, match="mha"):             # the kernels themselves refuse
        ops.mha_seq_forward(a["q"], a["k"], a["v"], a["lens"], heads)
