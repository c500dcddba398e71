"""The MFMA GEMM kernels against fp64 references, bit for bit.

Every operand is a small integer (biases: multiples of 0.25), so every
product and partial sum is an fp32 number and the fp32 result is unique
whatever the accumulation order, split or tile schedule; the one rounding
left, fp32 -> bf16, is deterministic (tests/gemm_exact.py, which also proves
on the CPU that the method catches a dropped K element, truncation and a
double rounding: tests/test_gemm_exact_reference.py).  Each case passes
assert_exact_inputs -- and assert_teeth where the output is bf16 -- before
it touches a kernel; outputs sit in sentinel-guarded buffers and inputs in
NaN-padded ones; every comparison is torch.equal."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import gemm_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


def _abi():
    from deeprec_amd import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream_handle, _lib.workspace


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ---------------------------------------------------------------------------
# gemm_nt: tile 128 x 128 x 64 (GM_BM, GM_BN, GM_BK in mlp.hip)
# ---------------------------------------------------------------------------
NT_SHAPES = [(1, 8, 64), (127, 120, 64), (129, 136, 128), (257, 264, 192), (128, 128, 1024)]
# Operands in [-r, r]: integers up to 256 are bf16 numbers, so the sums must
# pass 256 to be inexact.  sqrt(K) r (r + 1) / 3, their standard deviation,
# is about 500 here: bf16 steps of 2 and 4, where every 2nd / 4th integer is
# a tie, also after a ReLU or a mask has zeroed half or two thirds of them.
NT_RANGE = {64: 13, 128: 11, 192: 10, 1024: 6}


@functools.lru_cache(maxsize=None)
def nt_case(M, N, K, bias, act, device=DEV):
    """Inputs (CPU) and the fp32-exact reference (device) of one gemm_nt
    case; act ACT_MASK draws a mask.  Shared by the output types and the
    split-K factors."""
    r = NT_RANGE[K]

    def build(seed):
        g = X.gen(131 * M + 17 * N + K + 3 * act + (1 if bias else 0) + 100003 * seed)
        a, b = X.ints(g, (M, K), r), X.ints(g, (N, K), r)
        bb = X.quarters(g, N, 4) if bias else None
        mk = X.masks(g, (M, N)) if act == X.ACT_MASK else None
        da, db, dbb, dmk = [None if t is None else t.to(device) for t in (a, b, bb, mk)]
        ref, bound, q = X.gemm_nt_ref(da, db, dbb, act, dmk)
        X.assert_exact_inputs(bound, q, bf16=[t for t in (da, db, dmk) if t is not None],
                              multiples=[(da, 1.0), (db, 1.0)] + ([(dbb, 0.25)] if bias else []))
        return (a, b, bb, mk), X.to_f32(ref)

    return X.with_teeth(build, lambda c: c[1:])


def run_gemm_nt(a, b, bias, act, mask, out_fp32, split_k, lda=None, ldb=None, ldc=None,
                ld_aux=None):
    """dr_gemm_nt_bf16 (dr_gemm_nt_bf16_ex with a mask) on NaN-padded inputs
    and a guarded output."""
    lib, check, ptr, stream, workspace = _abi()
    M, K = a.shape
    N = b.shape[0]
    da, db = X.nan_padded(a, DEV, ld=lda), X.nan_padded(b, DEV, ld=ldb)
    dbias = None if bias is None else bias.to(DEV)
    out = X.Guarded(M, N, torch.float32 if out_fp32 else torch.bfloat16, DEV, ld=ldc)
    wsb = lib.dr_gemm_nt_workspace_size(M, N, split_k)
    ws = workspace(wsb, DEV) if wsb else None
    if mask is not None or act == X.ACT_MASK:
        dm = X.nan_padded(mask, DEV, ld=ld_aux)
        check(lib.dr_gemm_nt_bf16_ex(ptr(da), da.stride(0), ptr(db), db.stride(0), M, N, K,
                                     ptr(dbias), act, ptr(dm), dm.stride(0), ptr(out.view),
                                     out.ld, 1 if out_fp32 else 0, split_k, ptr(ws), wsb,
                                     stream(DEV)))
    else:
        check(lib.dr_gemm_nt_bf16(ptr(da), da.stride(0), ptr(db), db.stride(0), M, N, K,
                                  ptr(dbias), act, ptr(out.view), out.ld, 1 if out_fp32 else 0,
                                  split_k, ptr(ws), wsb, stream(DEV)))
    torch.cuda.synchronize(DEV)
    out.check("gemm_nt C")
    return out.view


def _nt_want(ref, out_fp32):
    return ref if out_fp32 else ref.to(torch.bfloat16)


@pytest.mark.parametrize("split_k", [1, 2, 3, 7])
@pytest.mark.parametrize("out_fp32", [False, True])
@pytest.mark.parametrize("act", [X.ACT_NONE, X.ACT_RELU])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_exact(M, N, K, bias, act, out_fp32, split_k):
    """Both sides of the M and N tile edges with one to sixteen K steps;
    split_k 7 exceeds K / 64 on the small shapes (clamped) and leaves an
    empty last chunk at K = 1024; 2 at K = 192 gives uneven chunks."""
    (a, b, bb, _), ref = nt_case(M, N, K, bias, act)
    got = run_gemm_nt(a, b, bb, act, None, out_fp32, split_k)
    X.assert_equal(got, _nt_want(ref, out_fp32), "gemm_nt (%d, %d, %d) split %d"
                   % (M, N, K, split_k))


@pytest.mark.parametrize("which", ["lda", "ldb", "ldc"])
@pytest.mark.parametrize("out_fp32", [False, True])
def test_gemm_nt_exact_strides(which, out_fp32):
    """One row stride at a time larger than K / N: the extra input columns
    hold NaNs, the extra output columns the sentinel."""
    M, N, K = 129, 136, 128
    (a, b, bb, _), ref = nt_case(M, N, K, True, X.ACT_NONE)
    ld = {"lda": dict(lda=K + 64), "ldb": dict(ldb=K + 8), "ldc": dict(ldc=N + 24)}[which]
    for split_k in (1, 2):
        got = run_gemm_nt(a, b, bb, X.ACT_NONE, None, out_fp32, split_k, **ld)
        X.assert_equal(got, _nt_want(ref, out_fp32), "gemm_nt %s split %d" % (which, split_k))


@pytest.mark.parametrize("out_fp32", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_mask_exact(M, N, K, bias, out_fp32):
    """ACT_MASK, the fused ReLU backward of every _MfmaMLP dx: masks over
    {-2, -1, -0.0, 0, 1, 3} with ld_aux > N; the output is zero exactly
    where mask <= 0."""
    (a, b, bb, mk), ref = nt_case(M, N, K, bias, X.ACT_MASK)
    got = run_gemm_nt(a, b, bb, X.ACT_MASK, mk, out_fp32, 1, ld_aux=N + 16)
    X.assert_equal(got, _nt_want(ref, out_fp32), "gemm_nt mask (%d, %d, %d)" % (M, N, K))
    off = mk.to(DEV).float() <= 0
    assert bool((got[off] == 0).all())
    assert bool((got[~off] != 0).any())


def test_gemm_nt_mask_refuses_split_k():
    from deeprec_amd._lib import InvalidArgumentError
    (a, b, bb, mk), _ = nt_case(129, 136, 128, True, X.ACT_MASK)
    with pytest.raises(InvalidArgumentError):
        run_gemm_nt(a, b, bb, X.ACT_MASK, mk, False, 2)


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("out_fp32", [False, True])
def test_gemm_nt_coded_identity(out_fp32, permuted):
    """A the (row-permuted) identity padded to [M, K], B[j][k] = ((3 j - 5 k)
    mod 17) - 8: C[i][j] = B[j][perm[i]], rows past K zero -- a transposed or
    permuted tile write is unmistakable.  (All values are bf16 numbers: this
    case is about placement, not rounding, so it has no teeth to assert.)"""
    M, N, K = 257, 264, 192
    perm = torch.randperm(K, generator=X.gen(5)) if permuted else torch.arange(K)
    a, b = X.coded_a(M, K, perm), X.coded_b(N, K)
    ref, bound, q = X.gemm_nt_ref(*_dev(a, b))
    X.assert_exact_inputs(bound, q, bf16=[a, b])
    want = torch.zeros(M, N, dtype=torch.float64)
    want[:K] = b.double().t()[perm]
    assert torch.equal(ref.cpu(), want)
    for split_k in (1, 2):
        got = run_gemm_nt(a, b, None, X.ACT_NONE, None, out_fp32, split_k)
        X.assert_equal(got, _nt_want(X.to_f32(ref), out_fp32), "gemm_nt coded split %d" % split_k)


# ---------------------------------------------------------------------------
# gemm_tn: tile 128 x 128, the rows in steps of 64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("colsum", [True, False])
@pytest.mark.parametrize("R,N,K,split", [(64, 8, 8, 1), (192, 136, 520, 2), (640, 72, 200, 3),
                                         (320, 128, 128, 4)])
def test_gemm_tn_exact(R, N, K, split, colsum):
    """dw = g^T x and colsum = column sums of g, fp32.  The row chunks are
    uneven (192 / 2 -> 128 + 64, 640 / 3 -> 256 + 256 + 128); at (320, 4)
    bchunk rounds up to 128 rows, so the entry recomputes S_ = 3.  g and x
    are column windows of wider matrices (NaNs on both sides), dw has a row
    stride larger than K."""
    gen = X.gen(R + 3 * N + 5 * K)
    g, x = X.ints(gen, (R, N), 13), X.ints(gen, (R, K), 13)
    dw, cs, top, q = X.gemm_tn_ref(*_dev(g, x))
    X.assert_exact_inputs(top, q, bf16=[g, x], multiples=[(g, 1.0), (x, 1.0)])
    lib, check, ptr, stream, workspace = _abi()
    dg = X.nan_padded(g, DEV, ld=N + 24, col_off=8)
    dx = X.nan_padded(x, DEV, ld=K + 16, col_off=16)
    out = X.Guarded(N, K, torch.float32, DEV, ld=K + 12)
    col = X.Guarded(1, N, torch.float32, DEV) if colsum else None
    wsb = lib.dr_gemm_tn_workspace_size(N, K, split, 1 if colsum else 0)
    ws = workspace(wsb, DEV) if wsb else None
    check(lib.dr_gemm_tn_bf16(ptr(dg), dg.stride(0), ptr(dx), dx.stride(0), R, N, K,
                              ptr(out.view), out.ld, ptr(col.view) if col else None, split,
                              ptr(ws), wsb, stream(DEV)))
    torch.cuda.synchronize(DEV)
    out.check("gemm_tn dw")
    X.assert_equal(out.view, X.to_f32(dw), "gemm_tn dw (%d, %d, %d) split %d" % (R, N, K, split))
    if colsum:
        col.check("gemm_tn colsum")
        X.assert_equal(col.view[0], X.to_f32(cs), "gemm_tn colsum")


# ---------------------------------------------------------------------------
# mlp_head: the N = 1 output layer; kHeadRows = 64 rows per backward block,
# 256 / (K / 8) rows per forward block
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_case(B, K, w_fp32, bias, device=DEV):
    """h: non-negative integers with exact zeros (the ReLU mask of h
    matters); w and grad_z integers in [-40, 40], so that grad_h = gz w
    passes 256.  The bf16 layer rounds z and grad_h; with w_fp32 the logit
    stays fp32."""
    def build(seed):
        g = X.gen(7 * B + K + (2 if w_fp32 else 0) + (1 if bias else 0) + 100003 * seed)
        h = X.relu_ints(g, (B, K), 3)
        w = X.ints(g, (K,), 40, dtype=torch.float32 if w_fp32 else torch.bfloat16)
        gz = X.ints(g, (B,), 40, dtype=torch.float32)
        bb = X.quarters(g, 1, 4) if bias else None
        dh, dw_, dbb, dgz = [None if t is None else t.to(device) for t in (h, w, bb, gz)]
        z, gh, dw, db, top, q = X.mlp_head_ref(dh, dw_, dbb, dgz)
        X.assert_exact_inputs(top, q, bf16=[dh, dw_, dgz],
                              multiples=[(dh, 1.0), (dw_, 1.0), (dgz, 1.0)] +
                              ([(dbb, 0.25)] if bias else []))
        assert bool((dh == 0).any()) and bool((dh > 0).any())
        return (h, w, bb, gz), X.to_f32(z), X.to_f32(gh), X.to_f32(dw), X.to_f32(db)

    return X.with_teeth(build, lambda c: (c[2],) if w_fp32 else (c[1], c[2]))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("w_fp32", [False, True])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
@pytest.mark.parametrize("K", [64, 128, 256, 512])
def test_mlp_head_exact(K, B, w_fp32, bias):
    (h, w, bb, gz), z, gh, dw, db = head_case(B, K, w_fp32, bias)
    lib, check, ptr, stream, _ = _abi()
    dh = X.nan_padded(h, DEV, ld=K + 8)
    dw_, dbb, dgz = _dev(w, bb, gz)
    zo = X.Guarded(B, 1, torch.float32, DEV)
    check(lib.dr_mlp_head_forward_bf16(ptr(dh), dh.stride(0), B, K, ptr(dw_), 1 if w_fp32 else 0,
                                       ptr(dbb), ptr(zo.view), stream(DEV)))
    P = lib.dr_mlp_head_grad_partials(B)
    assert P == (B + 63) // 64
    gho = X.Guarded(B, K, torch.bfloat16, DEV, ld=K + 8)
    dwp = X.Guarded(P, K, torch.float32, DEV)
    dbp = X.Guarded(P, 1, torch.float32, DEV)
    check(lib.dr_mlp_head_backward_bf16(ptr(dh), dh.stride(0), B, K, ptr(dw_),
                                        1 if w_fp32 else 0, ptr(dgz), ptr(gho.view), gho.ld,
                                        ptr(dwp.view), ptr(dbp.view), stream(DEV)))
    torch.cuda.synchronize(DEV)
    for gd, name in ((zo, "z"), (gho, "grad_h"), (dwp, "dw partials"), (dbp, "db partials")):
        gd.check("mlp_head " + name)
    # the bf16 layer's logit is a bf16 number held as fp32
    want_z = z if w_fp32 else z.to(torch.bfloat16).float()
    X.assert_equal(zo.view[:, 0], want_z, "mlp_head z (B=%d, K=%d)" % (B, K))
    X.assert_equal(gho.view, gh.to(torch.bfloat16), "mlp_head grad_h (B=%d, K=%d)" % (B, K))
    # the partials are sums of integers: fp32 adds them exactly in any order
    X.assert_equal(dwp.view.sum(0), dw, "mlp_head dw")
    X.assert_equal(dbp.view.sum(), db, "mlp_head db")


# ---------------------------------------------------------------------------
# crossnet_forward through the C entry (the 8-phase 256 x 256 kernel)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cross_case(B, d, bias):
    return X.crossnet_case(B, d, bias, DEV)


@pytest.mark.parametrize("with_lin", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("d", [64, 128, 256, 320])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 513])
def test_crossnet_forward_exact(B, d, bias, with_lin):
    """d: one K step, two K steps, one full column tile, a ragged column
    tile; B on both sides of the 256-row tile.  out = bf16(x0 * lin + xl)
    from the unrounded fp32 lin; lin = bf16(xl W^T + b)."""
    X.check_crossnet_forward(cross_case(B, d, bias), with_lin, DEV,
                             name="(B=%d, d=%d)" % (B, d))


def test_crossnet_forward_exact_production_width():
    """(257, 3392): 53 K steps and the 64-column remainder of the DCN width."""
    case = X.crossnet_case(257, 3392, True, DEV)
    X.check_crossnet_forward(case, True, DEV, name="(B=257, d=3392)")


def test_crossnet_forward_coded_permutation():
    """W a permutation matrix and x0 = 1: out = xl[:, perm] + b + xl and
    lin = xl[:, perm] + b, every value a bf16 number (placement, not
    rounding: no teeth to assert)."""
    B, d = 257, 320
    g = X.gen(11)
    perm = torch.randperm(d, generator=g)
    W = X.coded_a(d, d, perm)                      # W[o][perm[o]] = 1
    xl = X.ints(g, (B, d), 4)
    x0 = torch.ones(B, d, dtype=torch.bfloat16)
    b = X.quarters(g, d, 4)
    out, lin, bound, q = X.crossnet_ref(*_dev(x0, xl, W, b))
    X.assert_exact_inputs(bound, q, bf16=[x0, xl, W])
    want = xl.double()[:, perm] + b.double() + xl.double()
    assert torch.equal(out.cpu(), want)
    X.check_crossnet_forward(((x0, xl, W, b), X.to_f32(out), X.to_f32(lin)), True, DEV,
                             name="coded")


# ---------------------------------------------------------------------------
# crossnet_kernel, the general d % 8 fallback (dr_crossnet_layer_bf16)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B", [1, 127, 129])
@pytest.mark.parametrize("d", [8, 72, 200])
def test_crossnet_fallback_exact(d, B, bias):
    """d % 64 != 0: the entry takes crossnet_kernel (128 x 128 tiles, K steps
    of 32: 8 is a quarter step, 72 and 200 end on a quarter step)."""
    X.check_crossnet_forward(X.crossnet_case(B, d, bias, DEV), False, DEV, entry="layer",
                             name="fallback (B=%d, d=%d)" % (B, d))


@pytest.mark.parametrize("B", [1, 129])
def test_crossnet_fallback_unaligned_bias(B):
    """d = 128 with the bias pointer one float into its buffer: not 16-B
    aligned, so the entry must pick the fallback and still be right."""
    X.check_crossnet_forward(X.crossnet_case(B, 128, True, DEV), False, DEV, bias_offset=1,
                             name="unaligned bias (B=%d)" % B)


# ---------------------------------------------------------------------------
# crossnet_dx = bf16(u W + g), wt = W^T
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 256, 320])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 513])
def test_crossnet_dx_exact(B, d):
    X.check_crossnet_dx(X.crossnet_dx_case(B, d, DEV), DEV, name="(B=%d, d=%d)" % (B, d))


def test_crossnet_dx_exact_production_width():
    X.check_crossnet_dx(X.crossnet_dx_case(257, 3392, DEV), DEV, name="(B=257, d=3392)")


# ---------------------------------------------------------------------------
# crossnet_dw = u^T x in fp32, the batch in slices summed in slice order
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dw_case(B, d):
    g = X.gen(B + 7 * d)
    u, x = X.ints(g, (B, d), 4), X.ints(g, (B, d), 4)
    du, dx = _dev(u, x)
    want = du.double().t() @ dx.double()
    X.assert_exact_inputs(du.double().abs().t() @ dx.double().abs(), 1.0, bf16=[du, dx],
                          multiples=[(du, 1.0), (dx, 1.0)])
    return u, x, X.to_f32(want)


# crossnet_dw_slices(B, d): s slices need B / s >= 1024 and fill tiles * s /
# (rounds * 256) of the CUs at least 0.02 better than the best so far, tiles
# = ceil(d / 256)^2.  (64, 64) and (1024, 192): 1 slice.  (2048, 320) and
# (2112, 320): 4 tiles, s = 2 (8 / 256 against 4 / 256, which itself is
# below 0.02), s = 3 leaves under 1024 rows: 2 slices, ragged at 2112 (17 +
# 16 steps of 64 rows).  (6144, 64): 1 tile, s / 256 first passes 0.02 at
# s = 6 and 6144 / 7 < 1024: 6 slices.
@pytest.mark.parametrize("kernel,order", [("w4", "4"), ("w4", "0"), ("w4", "14"), ("w4", "xcd"),
                                          ("8ph", "4")])
@pytest.mark.parametrize("B,d", [(64, 64), (1024, 192), (2048, 320), (2112, 320), (6144, 64)])
def test_crossnet_dw_exact(B, d, kernel, order, monkeypatch):
    monkeypatch.setenv("DR_CROSSNET_DW_KERNEL", kernel)
    monkeypatch.setenv("DR_CROSSNET_DW_ORDER", order)
    u, x, want = dw_case(B, d)
    lib, check, ptr, stream, workspace = _abi()
    du, dx = X.nan_padded(u, DEV), X.nan_padded(x, DEV)
    dw = X.Guarded(d, d, torch.float32, DEV)
    wsb = lib.dr_crossnet_dw_workspace_size(B, d)
    ws = workspace(wsb, DEV)
    check(lib.dr_crossnet_dw_bf16(ptr(du), ptr(dx), B, d, ptr(dw.view), ptr(ws), wsb,
                                  stream(DEV)))
    torch.cuda.synchronize(DEV)
    dw.check("crossnet dw")
    X.assert_equal(dw.view, want, "crossnet dw (B=%d, d=%d) %s/%s" % (B, d, kernel, order))


# ---------------------------------------------------------------------------
# dot_interaction (f32 MFMA, LDS-tiled and per-pair kernels) and its backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,D", [(1, 2, 16), (5, 16, 32), (7, 17, 64), (9, 32, 128),
                                   (3, 27, 128),      # the MFMA kernel
                                   (4, 24, 96),       # the LDS-tiled kernel
                                   (6, 27, 12)])      # the per-pair kernel
def test_dot_interaction_exact(B, F, D):
    lib, check, ptr, stream, _ = _abi()
    x = X.ints(X.gen(B + 3 * F + D), (B, F, D), 4, dtype=torch.float32)
    want, bound, q = X.dot_ref(x.to(DEV))
    X.assert_exact_inputs(bound, q, multiples=[(x, 1.0)])
    dx = X.nan_padded(x, DEV)
    out = X.Guarded(B, F * (F - 1) // 2, torch.float32, DEV)
    check(lib.dr_dot_interaction(ptr(dx), B, F, D, ptr(out.view), stream(DEV)))
    torch.cuda.synchronize(DEV)
    out.check("dot_interaction out")
    X.assert_equal(out.view, X.to_f32(want), "dot_interaction (%d, %d, %d)" % (B, F, D))


@pytest.mark.parametrize("D", [4, 16, 128])
@pytest.mark.parametrize("B", [1, 7, 9])
@pytest.mark.parametrize("F", [2, 16, 17, 28, 29, 32])
def test_dot_interaction_grad_exact(F, B, D):
    """The dot_grad_kernel<16 / 28 / 32> edges, B around the eight rows of
    a block."""
    lib, check, ptr, stream, _ = _abi()
    g = X.gen(F + 5 * B + 11 * D)
    x = X.ints(g, (B, F, D), 4, dtype=torch.float32)
    tg = X.ints(g, (B, F * (F - 1) // 2), 4, dtype=torch.float32)
    want, bound, q = X.dot_grad_ref(x.to(DEV), tg.to(DEV))
    X.assert_exact_inputs(bound, q, multiples=[(x, 1.0), (tg, 1.0)])
    dx, dtg = X.nan_padded(x, DEV), X.nan_padded(tg, DEV)
    out = X.Guarded(B, F * D, torch.float32, DEV)
    check(lib.dr_dot_interaction_grad(ptr(dx), ptr(dtg), B, F, D, ptr(out.view), stream(DEV)))
    torch.cuda.synchronize(DEV)
    out.check("dot_interaction_grad grad_x")
    X.assert_equal(out.view.reshape(B, F, D), X.to_f32(want),
                   "dot_interaction_grad (%d, %d, %d)" % (B, F, D))


# ---------------------------------------------------------------------------
# The CrossNet kernels that an environment variable selects, read once per
# process: one fresh child process each (python tests/gemm_exact.py crossnet)
# ---------------------------------------------------------------------------
# 1 falls through to crossnet_glds_kernel; 3 glds3, 4 the 256^2 kernel, 5
# stag, 6 / 9 / 10 the 8-phase kernel in other tile orders / epilogue, 12 the
# 8-phase kernel plus the glds kernel on the d % 256 strip, 14 / 16 the
# one-wave-per-SIMD kernel (also in dx).  Left out: 7, 15 and 17, timing-only
# builds that write no output, and 11, which launches the default's kernel.
VARIANTS = [("DR_CROSSNET_LEGACY", "1")] + [("DR_CROSSNET_VARIANT", str(v))
                                            for v in (1, 3, 4, 5, 6, 9, 10, 12, 14, 16)]
ABNORMAL_STATUS = (124, 134, 137, 139)
_abnormal = []          # set once a child ended abnormally: nothing more is started


@pytest.mark.parametrize("var,value", VARIANTS)
def test_crossnet_env_variant_exact(var, value):
    """The forward at (257, 320) and (513, 64) and dx at (257, 320) under one
    variant, in a child of its own (never more than one at a time); the
    child prints the mismatch reports and exits 0 or 1.  A kernel that has
    faulted is not followed by further launches: once a child was killed by
    a signal, ended with 124 / 134 / 137 / 139 or ran into the timeout, the
    remaining variants fail at once without starting anything."""
    if _abnormal:
        pytest.fail("not run: an earlier variant ended abnormally (%s)" % _abnormal[0])
    env = {**os.environ, var: value}
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "gemm_exact.py"), "crossnet"],
                           env=env, timeout=180, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _abnormal.append("%s=%s: timeout" % (var, value))
        pytest.fail("%s=%s: the child ran into the timeout\n%s" % (var, value, e.stdout))
    if p.returncode < 0 or p.returncode in ABNORMAL_STATUS:
        _abnormal.append("%s=%s: status %d" % (var, value, p.returncode))
    assert p.returncode == 0, "%s=%s: exit status %d\n%s" % (var, value, p.returncode, p.stdout)
