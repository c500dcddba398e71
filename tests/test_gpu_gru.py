"""The GRU / AUGRU sequence kernels (csrc/gru.hip) against
the tests' own fp64 step loop (gru_ref.py), and the exactness properties the
kernels promise: zeros past seq_len, a row's result independent of the rows
around it and of the padded length, att = 0 is the plain GRU, att = 1 copies
the candidate, run-to-run equality, and a one-stream capture.

Bounds: out, h_final, grad_xp and grad_att within rtol = atol = 1e-5 of the
fp64 reference (the project's kernel bound, test_gpu_din.py).  The state-
weight, input-weight and bias gradients sum B * T position terms: an fp32
torch twin of the reference reaches 0.78 of that bound at (37, 100, 36) on its
own, so for those the native path may err by the larger of the bound and 4 x
the twin's own error on the same inputs (another summation order may be a few
times worse, not orders of magnitude)."""
import pytest
import torch

import gru_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, T, H, I): B not a multiple of the 16-row block, a lone row, T = 1, the
# widest and the narrowest native H
SHAPES = [(37, 100, 36, 36), (17, 65, 36, 36), (5, 150, 64, 64), (33, 23, 20, 12), (9, 7, 4, 4),
          (3, 1, 36, 36), (1, 100, 36, 36)]


@pytest.mark.parametrize("use_att", [False, True])
@pytest.mark.parametrize("B,T,H,I", SHAPES)
def test_gru_sequence_matches_fp64(B, T, H, I, use_att):
    from deeprec_amd import ops
    cs, ref, twin = gru_ref.reference(B, T, H, use_att, I)
    assert ops._GRU_NATIVE and ops.gru_native_ok(torch.empty(B, T, 3 * H, device=DEV))
    got = gru_ref.run(cs, ops.gru_sequence, torch.float32, DEV, use_att)
    report = []
    for name in gru_ref.NAMES:
        if ref[name] is None:
            continue
        e, te = gru_ref.ratio(got[name], ref[name]), gru_ref.ratio(twin[name], ref[name])
        report.append("%s %.3f (twin %.3f)" % (name, e, te))
    print("gru B=%d T=%d H=%d att=%d: error / bound: %s" % (B, T, H, use_att, ", ".join(report)))
    for name in gru_ref.NAMES:
        if ref[name] is None:
            continue
        e, te = gru_ref.ratio(got[name], ref[name]), gru_ref.ratio(twin[name], ref[name])
        limit = max(1.0, 4.0 * te) if name in gru_ref.SUMMED else 1.0
        assert e <= limit, (name, e, te)


def _inputs(B, T, H, I, use_att, rows=None, pad=0):
    """fp32 device inputs of the kernels for the case of a shape: rows picks
    batch rows, pad appends steps (random values a kernel must not use)."""
    cs = gru_ref.reference(B, T, H, use_att, I)[0]
    f = lambda k: cs[k].float()  # noqa: E731
    xp = f("x") @ torch.cat([f("Wg")[:I], f("Wc")[:I]], 1) + torch.cat([f("bg"), f("bc")])
    att, go, gh, lens = f("att"), f("go"), f("gh"), cs["lens"].to(torch.int32)
    if pad:
        g = torch.Generator().manual_seed(pad)
        xp = torch.cat([xp, torch.randn(B, pad, 3 * H, generator=g)], 1)
        att = torch.cat([att, torch.rand(B, pad, generator=g)], 1)
        go = torch.cat([go, torch.randn(B, pad, H, generator=g)], 1)
    if rows is not None:
        xp, att, go, gh, lens = (t[rows] for t in (xp, att, go, gh, lens))
    d = lambda t: t.contiguous().to(DEV)  # noqa: E731
    return dict(xp=d(xp), wg=d(f("Wg")[I:]), wc=d(f("Wc")[I:]), lens=d(lens),
                att=d(att) if use_att else None, go=d(go), gh=d(gh))


def _native(a):
    """(out, h_final, saved, grad_xp, grad_att) of the two kernels."""
    from deeprec_amd import ops
    out, hf, saved = ops.gru_seq_forward(a["xp"], a["wg"], a["wc"], a["lens"], a["att"])
    gxp, ga = ops.gru_seq_backward(a["wg"], a["wc"], a["lens"], a["att"], out, saved, a["go"],
                                   a["gh"])
    return out, hf, saved, gxp, ga


def _first(res, T):
    """The first T steps of a run over a longer padded length."""
    out, hf, saved, gxp, ga = res
    return out[:, :T], hf, saved[:, :T], gxp[:, :T], None if ga is None else ga[:, :T]


def _same(xs, ys):
    for x, y in zip(xs, ys):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y)


@pytest.mark.parametrize("use_att", [False, True])
@pytest.mark.parametrize("B,T,H,I", SHAPES)
def test_padded_steps_are_exact_zeros_and_runs_repeat(B, T, H, I, use_att):
    a = _inputs(B, T, H, I, use_att)
    out, hf, saved, gxp, ga = _native(a)
    pad = torch.arange(T, device=DEV)[None, :] >= a["lens"][:, None]
    zero = lambda t: torch.equal(t[pad], torch.zeros_like(t[pad]))  # noqa: E731
    assert zero(out) and zero(gxp) and zero(saved)
    assert ga is None or zero(ga)
    assert int(a["lens"][0]) == T
    if B > 1:                                        # an empty row
        assert int(a["lens"][1]) == 0
        assert torch.equal(hf[1], torch.zeros(H, device=DEV))
    valid = ~pad
    last = (a["lens"].long() - 1).clamp(min=0)
    want_hf = out[torch.arange(B, device=DEV), last] * (a["lens"] > 0)[:, None]
    assert torch.equal(hf, want_hf)
    assert torch.isfinite(out).all() and torch.isfinite(gxp).all()
    if valid.any():
        assert float(gxp[valid].abs().max()) > 0
    _same(_native(a), (out, hf, saved, gxp, ga))     # two runs give equal results


@pytest.mark.parametrize("use_att", [False, True])
@pytest.mark.parametrize("B,T,H,I", [(37, 100, 36, 36), (17, 65, 36, 36), (33, 23, 20, 12)])
def test_a_row_does_not_depend_on_its_batch_or_the_padded_length(B, T, H, I, use_att):
    full = _native(_inputs(B, T, H, I, use_att))
    longer = _native(_inputs(B, T, H, I, use_att, pad=9))
    _same(_first(longer, T), full)                   # 9 more padded steps: the first T equal
    for b in (0, 16, B - 1):
        one = _native(_inputs(B, T, H, I, use_att, rows=slice(b, b + 1)))
        _same(one, [None if x is None else x[b:b + 1] for x in full])
        one9 = _native(_inputs(B, T, H, I, use_att, rows=slice(b, b + 1), pad=9))
        _same(_first(one9, T), one)


@pytest.mark.parametrize("B,T,H,I", [(37, 100, 36, 36), (5, 150, 64, 64), (9, 7, 4, 4)])
def test_att_zero_is_the_plain_gru_and_att_one_copies_the_candidate(B, T, H, I):
    plain = _native(_inputs(B, T, H, I, False))
    a = _inputs(B, T, H, I, True)
    a["att"] = torch.zeros_like(a["att"])
    zero = _native(a)
    _same(zero[:4], plain[:4])
    a["att"] = torch.ones_like(a["att"])
    out, hf, saved, gxp, ga = _native(a)
    valid = torch.arange(T, device=DEV)[None, :] < a["lens"][:, None]
    assert torch.equal(out[valid], saved[..., 2 * H:][valid])
    assert torch.equal(gxp[..., H:2 * H], torch.zeros_like(out))     # u' = 0: no update-gate path


def test_forward_and_backward_capture_on_one_stream():
    B, T, H, I = 17, 65, 36, 36
    for use_att in (False, True):
        a = _inputs(B, T, H, I, use_att)
        eager = _native(a)                              # warm-up, and the result to match
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                       # one stream, no parallel branches
            captured = _native(a)
        for t in captured:
            if t is not None:
                t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _same(captured, eager)


@pytest.mark.parametrize("use_att", [False, True])
def test_torch_arm_on_the_gpu_matches_fp64(use_att):
    """DR_GRU=torch selects ops._gru_sequence_torch at import; here it is
    called directly (the switch cannot change inside a process)."""
    from deeprec_amd import ops
    B, T, H, I = 17, 65, 36, 36
    cs, ref, _ = gru_ref.reference(B, T, H, use_att, I)
    got = gru_ref.run(cs, ops._gru_sequence_torch, torch.float32, DEV, use_att)
    for name in ("out", "hT", "dxp", "datt"):
        if ref[name] is not None:
            assert gru_ref.ratio(got[name], ref[name]) <= 1.0, name


def test_widths_outside_the_native_set_take_the_torch_composition():
    from deeprec_amd import ops
    for H in (6, 68):
        xp = torch.randn(3, 4, 3 * H, device=DEV)
        assert not ops.gru_native_ok(xp)
        out, hf = ops.gru_sequence(xp, torch.randn(H, 2 * H, device=DEV) * 0.1,
                                   torch.randn(H, H, device=DEV) * 0.1,
                                   torch.tensor([4, 0, 2], device=DEV))
        assert out.shape == (3, 4, H) and torch.equal(hf[1], torch.zeros(H, device=DEV))
    with pytest.raises(Exception, match="gru"):         # the kernels themselves refuse
        ops.gru_seq_forward(torch.zeros(3, 4, 18, device=DEV), torch.zeros(6, 12, device=DEV),
                            torch.zeros(6, 6, device=DEV), torch.tensor([1, 2, 3], device=DEV))
