"""The pooled lookup and its backward over every row-width class and every
bag-length path (tests/pool_sweep.py; the sweep itself is proved on the CPU by
tests/test_pool_sweep_ref.py).  Every result is compared with the CPU oracle
-- bit for bit unless the test says otherwise -- and must lie within the
rounding-count bound of a float64 restatement; sum pools of integer-valued
tables must equal the int64 sums exactly."""
import functools

import numpy as np
import pytest
import torch

import pool_sweep as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5          # against the oracle under max_norm (the norm is summed in another order)
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    deeprec_amd.load()
    deeprec_amd.set_validate(True)
    assert torch.cuda.is_available()
    return deeprec_amd


@pytest.fixture(scope="module")
def ops(dr):
    from deeprec_amd import ops
    return ops


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), device=DEV, dtype=dtype)


def H(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def finish(dr):
    torch.cuda.synchronize()
    dr.status_check()


def same_bits(got, want):
    np.testing.assert_array_equal(bits(got), bits(want))


@functools.lru_cache(maxsize=None)
def fref(dim, kind, seq, comb, weighted, clipped, bf16=False):
    """The float64 reference of one forward case, computed once."""
    c = (S.bf16_case if bf16 else S.seq_case if seq else S.forward_case)(dim, kind)
    table = c.table
    if bf16:
        from oracle import oracle as orc
        table = orc.bf16_round(table)
    return S.forward_ref(table, c.ids, c.off, comb, c.weights if weighted else None,
                         c.max_norm if clipped else None)


def sparse(dr, c, values):
    return dr.SparseTensor(T(c.ind), T(values), (c.B, int(c.lens.max())))


# ---------------------------------------------------------------------------
# Forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.POOL_WIDTHS)
def test_forward_ali(dr, ops, orc, dim):
    """ops.sparse_segment_{sum,mean,sqrt_n}: dispatch_pool<ORDER_ALI>, the fast
    kernel on the chunk of one-id bags, the general kernel on the rest."""
    c, ci = S.forward_case(dim), S.forward_case(dim, "int")
    fns = {"sum": ops.sparse_segment_sum, "mean": ops.sparse_segment_mean,
           "sqrtn": ops.sparse_segment_sqrt_n}
    table, idx, seg = T(c.table), T(c.ids, torch.int32), T(c.seg)
    for comb in S.COMBINERS:
        got = H(fns[comb](table, idx, seg, num_segments=c.B))
        same_bits(got, orc.sparse_segment_reduce(c.table, c.ids, c.seg, comb, num_segments=c.B))
        S.within(got, *fref(dim, "rand", False, comb, False, False))
    got = H(ops.sparse_segment_sum(T(ci.table), T(ci.ids, torch.int32), T(ci.seg),
                                   num_segments=ci.B))
    np.testing.assert_array_equal(got.astype(np.int64), S.int_sum_ref(ci.table, ci.ids, ci.off))
    finish(dr)


@pytest.mark.parametrize("dim", S.POOL_WIDTHS)
def test_forward_seq(dr, ops, orc, dim):
    """ops.fused_embedding_local_sparse_look_up: dispatch_pool<ORDER_SEQ>, with
    and without max_norm."""
    c, k, ci = S.seq_case(dim), S.seq_case(dim, "clip"), S.seq_case(dim, "int")
    shape = (c.B, int(c.lens.max()))
    table, ktable, ids, ind = T(c.table), T(k.table), T(c.ids), T(c.ind)
    for comb in S.COMBINERS:
        got, off = ops.fused_embedding_local_sparse_look_up(ids, ind, shape, table, comb)
        ref, roff = orc.fused_local_lookup(c.table, c.ids, c.seg, c.B, comb)
        same_bits(H(got), ref)
        np.testing.assert_array_equal(H(off), roff)
        S.within(H(got), *fref(dim, "rand", True, comb, False, False))
        got, _ = ops.fused_embedding_local_sparse_look_up(T(k.ids), T(k.ind), shape, ktable, comb,
                                                          k.max_norm)
        ref, _ = orc.fused_local_lookup(k.table, k.ids, k.seg, k.B, comb, k.max_norm)
        np.testing.assert_allclose(H(got), ref, rtol=RTOL)
        S.within(H(got), *fref(dim, "clip", True, comb, False, True))
    got, _ = ops.fused_embedding_local_sparse_look_up(T(ci.ids), T(ci.ind), shape, T(ci.table),
                                                      "sum")
    np.testing.assert_array_equal(H(got).astype(np.int64),
                                  S.int_sum_ref(ci.table, ci.ids, ci.off))
    finish(dr)


@pytest.mark.parametrize("dim", S.POOL_WIDTHS)
def test_forward_weighted_and_clipped(dr, orc, dim):
    """embedding_lookup_sparse on a dense table with sp_weights (the empty
    weighted mean / sqrtn bag is NaN, as the reference's), and with max_norm
    at the ragged widths, where the norm's lane sum meets idle lanes."""
    c, k, ci = S.forward_case(dim), S.forward_case(dim, "clip"), S.forward_case(dim, "int")
    table, sp, spw = T(c.table), sparse(dr, c, c.ids), sparse(dr, c, c.weights)
    for comb in S.COMBINERS:
        got = H(dr.embedding_lookup_sparse(table, sp, spw, combiner=comb))
        ref = orc.embedding_lookup_sparse(c.table, c.ind, c.ids, c.B, c.weights, comb)
        assert np.isnan(got[8]).all() == (comb != "sum") and c.lens[8] == 0
        same_bits(got, ref)
        S.within(got, *fref(dim, "rand", False, comb, True, False))
    got = H(dr.embedding_lookup_sparse(T(ci.table), sparse(dr, ci, ci.ids),
                                       sparse(dr, ci, ci.weights), combiner="sum"))
    np.testing.assert_array_equal(got.astype(np.int64),
                                  S.int_sum_ref(ci.table, ci.ids, ci.off, ci.weights))
    if dim in S.MAXNORM_WIDTHS:
        ktable, ksp, kw = T(k.table), sparse(dr, k, k.ids), sparse(dr, k, k.weights)
        for comb in S.COMBINERS:
            for weighted in (False, True):
                got = H(dr.embedding_lookup_sparse(ktable, ksp, kw if weighted else None,
                                                   combiner=comb, max_norm=k.max_norm))
                ref = orc.embedding_lookup_sparse(k.table, k.ind, k.ids, k.B,
                                                  k.weights if weighted else None, comb,
                                                  k.max_norm)
                np.testing.assert_allclose(got, ref, rtol=RTOL)
                S.within(got, *fref(dim, "clip", False, comb, weighted, True))
    finish(dr)


def _desc(_lib, table, rows, ids, out_ptr, out_stride, bag_off=None, combiner=0):
    d = _lib.DrPoolDesc()
    d.pool, d.pool_rows, d.ids = table.data_ptr(), rows, ids.data_ptr()
    d.bag_off = None if bag_off is None else bag_off.data_ptr()
    d.out, d.out_stride, d.combiner, d.max_norm = out_ptr, out_stride, combiner, -1.0
    return d


@pytest.mark.parametrize("order", ["ali", "seq"])
@pytest.mark.parametrize("dim", S.POOL_WIDTHS)
def test_forward_onehot(dr, ops, orc, dim, order):
    """pool_onehot_kernel: 3 tables into one [B, 3 * D] concat, 3 * B no
    multiple of kOneHotNB = 4.  A plain gather; the fused op's order (0 + e)
    turns -0.0 into +0.0, the ALI order keeps it."""
    from deeprec_amd import _lib
    B, F = 11, 3
    rng = np.random.default_rng(dim)
    out = torch.full((B, F * dim), SENTINEL, device=DEV)
    tables, idss, descs, keep = [], [], [], []
    for t in range(F):
        tab = rng.standard_normal((S.TABLE_ROWS, dim)).astype(np.float32)
        tab[rng.random(tab.shape) < 0.1] = -0.0
        ids = rng.integers(0, S.TABLE_ROWS, B).astype(np.int64)
        dt, di = T(tab), T(ids)
        keep += [dt, di]
        tables.append(tab)
        idss.append(ids)
        descs.append(_desc(_lib, dt, S.TABLE_ROWS, di, out.data_ptr() + 4 * t * dim, F * dim))
    ops.pool_grouped(descs, B, dim, order=_lib.ORDER_SEQ if order == "seq" else _lib.ORDER_ALI,
                     onehot=True)
    got = H(out)
    for t in range(F):
        want = orc.gather(tables[t], idss[t])
        assert np.signbit(want[want == 0]).any()
        if order == "seq":
            want = want + np.float32(0.0)
            assert not np.signbit(want[want == 0]).any()
        same_bits(got[:, t * dim:(t + 1) * dim], want)
    finish(dr)


def _bf16_tensor(orc, a):
    return T(orc.bf16_bits(a).view(np.int16)).view(torch.bfloat16)


@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("dim", S.BF16_WIDTHS)
def test_forward_bf16(dr, ops, orc, dim, out_bf16):
    """Dense bf16 tables through dr_pool_grouped_ex (DR_POOL_BF16): one-hot
    slots and one-id chunks are bit copies (exact widenings into fp32),
    multi-hot bags pool the widened rows in fp32 and round once for a bf16
    output."""
    from deeprec_amd import _lib
    c, ci = S.bf16_case(dim), S.bf16_case(dim, "int")
    wide = orc.bf16_round(c.table)
    table, ids, off = _bf16_tensor(orc, c.table), T(c.ids), T(c.off)
    odt = torch.bfloat16 if out_bf16 else torch.float32

    def result(o):
        return H(o.float())

    for comb in S.COMBINERS:
        out = torch.full((c.B, dim), SENTINEL, device=DEV, dtype=odt)
        d = _desc(_lib, table, S.TABLE_ROWS, ids, out.data_ptr(), dim, off,
                  _lib.COMBINERS[comb])
        ops.pool_grouped([d], c.B, dim, bf16=True, out_bf16=out_bf16)
        got = result(out)
        ref = orc.sparse_segment_reduce(wide, c.ids, c.seg, comb, num_segments=c.B)
        same_bits(got[:8], wide[c.ids[:8]])            # the fast kernel's chunk: copies
        same_bits(got, orc.bf16_round(ref) if out_bf16 else ref)
        r64, bound = fref(dim, "rand", False, comb, False, False, True)
        if out_bf16:     # one more rounding, half an ulp of bf16's 8 bits
            bound = bound + 2.0 ** -8 * (np.abs(r64) + bound)
        S.within(got, r64, bound)
    if not out_bf16:
        out = torch.full((ci.B, dim), SENTINEL, device=DEV)
        d = _desc(_lib, _bf16_tensor(orc, ci.table), S.TABLE_ROWS, T(ci.ids), out.data_ptr(), dim,
                  T(ci.off))
        ops.pool_grouped([d], ci.B, dim, bf16=True)
        np.testing.assert_array_equal(H(out).astype(np.int64),
                                      S.int_sum_ref(ci.table, ci.ids, ci.off))
    B = 11                                              # one-hot: bag b is id b
    out = torch.full((B, dim), SENTINEL, device=DEV, dtype=odt)
    d = _desc(_lib, table, S.TABLE_ROWS, ids, out.data_ptr(), dim)
    ops.pool_grouped([d], B, dim, onehot=True, bf16=True, out_bf16=out_bf16)
    same_bits(result(out), wide[c.ids[:B]])
    finish(dr)


# ---------------------------------------------------------------------------
# Backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.CSR_WIDTHS)
def test_segment_grad_and_unsorted_segment_sum(dr, ops, orc, dim):
    """dispatch_csr_sum through SparseSegment*Grad and UnsortedSegmentSum
    (negative segment ids are skipped)."""
    c = S.backward_case(dim)
    fns = {"sum": ops.sparse_segment_sum_grad, "mean": ops.sparse_segment_mean_grad,
           "sqrtn": ops.sparse_segment_sqrt_n_grad}
    grad, idx, seg = T(c.grad), T(c.idx), T(c.seg)
    for comb in S.COMBINERS:
        got = H(fns[comb](grad, idx, seg, c.U))
        same_bits(got, orc.sparse_segment_reduce_grad(c.grad, c.idx, c.seg, c.U, comb))
        S.within(got, *S.segment_grad_ref(c.grad, c.idx, c.seg, c.lens, c.U, comb))
    got = H(ops.sparse_segment_sum_grad(T(c.int_grad), idx, seg, c.U))
    want = np.zeros((c.U, dim), np.int64)
    np.add.at(want, c.idx, c.int_grad.astype(np.int64)[c.seg])
    np.testing.assert_array_equal(got.astype(np.int64), want)
    useg = c.idx.copy()
    useg[::5] = -1 - (np.arange(useg[::5].size) % 3).astype(np.int32)
    data = c.grad[c.seg]
    got = H(ops.unsorted_segment_sum(T(data), T(useg), c.U + 2))
    same_bits(got, orc.unsorted_segment_sum(data, useg, c.U + 2))
    S.within(got, *S.unsorted_segment_sum_ref(data, useg, c.U + 2))
    assert not got[c.U:].any()
    finish(dr)


@pytest.mark.parametrize("dim", S.GRAD_WIDTHS)
def test_grouped_unique_backward(dr, orc, dim):
    """dr_pool_grad_grouped (the Unique path: a trainable plain tensor): the
    dense gradient holds the reference's per-unique-id rows, zeros elsewhere."""
    c = S.backward_case(dim)
    rng = np.random.default_rng(dim)
    table_np = rng.standard_normal((S.TABLE_ROWS, dim)).astype(np.float32)
    sp, spw = sparse(dr, c, c.ids), sparse(dr, c, c.weights)
    for comb, weighted in (("sum", False), ("mean", False), ("sqrtn", False), ("mean", True)):
        table = T(table_np).requires_grad_(True)
        out = dr.embedding_lookup_sparse(table, sp, spw if weighted else None, combiner=comb)
        out.backward(T(c.grad))
        w = c.weights if weighted else None
        uids, gref = orc.embedding_lookup_sparse_grad(table_np, c.ind, c.ids, c.B, c.grad, w, comb)
        np.testing.assert_array_equal(uids, c.uids)
        got = H(table.grad)
        same_bits(got[uids], gref)
        assert not np.delete(got, uids, 0).any()
        if weighted:
            S.within(got[uids], *S.weighted_grad_ref(c.grad, c.idx, c.seg, w, c.off, c.U, comb))
        else:
            S.within(got[uids], *S.segment_grad_ref(c.grad, c.idx, c.seg, c.lens, c.U, comb))
    finish(dr)


def _check_rows_slices(orc, c, sl, comb, weighted, grad):
    w = c.weights if weighted else None
    uids, gref = orc.embedding_lookup_sparse_grad(None, c.ind, c.ids, c.B, grad, w, comb)
    n = int(sl.num_valid.item())
    assert n == c.U
    np.testing.assert_array_equal(H(sl.indices[:n]), uids)
    got = H(sl.values[:n])
    same_bits(got, gref)
    if weighted:
        S.within(got, *S.weighted_grad_ref(grad, c.idx, c.seg, w, c.off, c.U, comb))
    else:
        S.within(got, *S.segment_grad_ref(grad, c.idx, c.seg, c.lens, c.U, comb))


ROWS_COMBOS = (("sum", False), ("mean", False), ("sqrtn", False), ("sum", True), ("mean", True),
               ("sqrtn", True))


@pytest.mark.parametrize("dim", [w for w in S.ROWS_WIDTHS if S.pool_class(w)])
def test_rows_backward(dr, orc, dim):
    """dr_pool_grad_rows_grouped_ex2 through an EV lookup and backward: the
    IndexedSlices are the reference's, unique ids in first-occurrence order."""
    c = S.backward_case(dim)
    sp, spw = sparse(dr, c, c.ids), sparse(dr, c, c.weights)
    for comb, weighted in ROWS_COMBOS:
        ev = dr.EmbeddingVariable("sweep_rows_%d_%s_%d" % (dim, comb, weighted), dim, 0.125,
                                  capacity=512)
        out = dr.embedding_lookup_sparse(ev, sp, spw if weighted else None, combiner=comb)
        out.backward(T(c.grad))
        _check_rows_slices(orc, c, ev.pending_grads.pop(), comb, weighted, c.grad)
    finish(dr)


@pytest.mark.parametrize("dim", [w for w in S.ROWS_WIDTHS if not S.pool_class(w)])
def test_rows_backward_wide_unaligned(dr, orc, dim):
    """The <1, 64, 16> class (unaligned rows of 257 .. 1023 floats), which no
    pooled forward reaches: the lookup's own steps -- resolve the ids into the
    EV, then the row-grouped backward over the resolved rows -- without the
    pool launch in between."""
    from deeprec_amd import embedding_ops as eo
    c = S.backward_case(dim)
    grad = T(c.grad)
    for comb, weighted in ROWS_COMBOS:
        ev = dr.EmbeddingVariable("sweep_rowsw_%d_%s_%d" % (dim, comb, weighted), dim, 0.125,
                                  capacity=512)
        f = eo._Feature(ev, T(c.ids), T(c.seg.astype(np.int64)), c.B,
                        T(c.weights) if weighted else None, comb, None, onehot=False)
        assert eo._rows_eligible([f])
        eo._prepare_group([f], need_grad=True)
        (sl,) = f.group.grads(grad, [0], dim)
        _check_rows_slices(orc, c, sl, comb, weighted, c.grad)
    finish(dr)


@pytest.mark.parametrize("dim,aligned", S.GATHER_CASES)
def test_gather(dr, ops, orc, dim, aligned):
    """dr_gather; an unaligned table (4 bytes past a 16-byte boundary) takes
    the scalar classes."""
    c = S.make_case(dim, 64, "rand")
    buf = torch.zeros(S.TABLE_ROWS * dim + 4, device=DEV)
    table = buf[0 if aligned else 1:][:S.TABLE_ROWS * dim].view(S.TABLE_ROWS, dim)
    table.copy_(T(c.table))
    assert table.is_contiguous() and (table.data_ptr() % 16 == 0) == aligned
    ids = c.ids[:203]                                   # no multiple of the 4 rows per group
    same_bits(H(ops.gather(table, T(ids))), orc.gather(c.table, ids))
    finish(dr)


@pytest.mark.parametrize("dim", sorted(set(S.CLIP_GRAD_WIDTHS) | set(S.MAXNORM_WIDTHS)))
def test_clip_by_norm_grad(dr, ops, orc, dim):
    """dr_clip_by_norm_grad: within the float64 bound, and within twice the
    bound of the oracle, which sums the norm and the dot product serially
    where the kernel sums across lanes."""
    k = S.forward_case(dim, "clip") if S.pool_class(dim) else S.make_case(dim, 64, "clip")
    rows = np.arange(7, 71, dtype=np.int64)
    g = np.random.default_rng(dim).standard_normal((rows.size, dim)).astype(np.float32)
    got = H(ops.clip_by_norm_grad(T(g), T(k.table), T(rows), k.max_norm,
                                  pool_rows=S.TABLE_ROWS))
    ref, bound = S.clip_by_norm_grad_ref(k.table[rows], g, k.max_norm)
    S.within(got, ref, bound)
    S.within(got, orc.clip_by_norm_grad(k.table[rows], g, k.max_norm).astype(np.float64),
             2 * bound)
    finish(dr)


# ---------------------------------------------------------------------------
# Refusals: the first width past every ladder
# ---------------------------------------------------------------------------
def _untouched(t):
    assert bool((t.float() == SENTINEL).all())


@pytest.mark.parametrize("dim,order,bf16", [(1028, "ali", False), (257, "ali", False),
                                            (1028, "seq", False), (257, "seq", False),
                                            (1032, "ali", True)])
def test_forward_refuses_the_next_width(dr, ops, dim, order, bf16):
    from deeprec_amd import _lib
    fn = S.pool_class_bf16 if bf16 else S.pool_class
    assert fn(dim) is None and fn(dim - (8 if bf16 else 4 if dim % 4 == 0 else 1)) is not None
    B = 5
    table = torch.zeros((8, dim), device=DEV, dtype=torch.bfloat16 if bf16 else torch.float32)
    ids = torch.arange(B, device=DEV)
    off = torch.arange(B + 1, device=DEV, dtype=torch.int32)
    for onehot in (False, True):
        out = torch.full((B, dim), SENTINEL, device=DEV)
        d = _desc(_lib, table, 8, ids, out.data_ptr(), dim, None if onehot else off)
        with pytest.raises(dr.DeepRecError):
            ops.pool_grouped([d], B, dim, order=_lib.ORDER_SEQ if order == "seq" else
                             _lib.ORDER_ALI, onehot=onehot, bf16=bf16)
        _untouched(out)
    finish(dr)


@pytest.mark.parametrize("dim", [1028, 257])
def test_csr_sum_refuses_the_next_width(dr, dim):
    from deeprec_amd._lib import check, lib, ptr, stream_handle, workspace
    assert S.csr_class(dim) is None
    n, U = 6, 4
    data = torch.ones((n, dim), device=DEV)
    seg = T(np.array([0, 1, 1, 3, 0, 2], np.int32))
    out = torch.full((U, dim), SENTINEL, device=DEV)
    wsb = lib().dr_unsorted_segment_sum_workspace_size(n, U)
    ws = workspace(wsb, DEV)
    with pytest.raises(dr.DeepRecError):
        check(lib().dr_unsorted_segment_sum(ptr(data), n, dim, ptr(seg), U, ptr(out), ptr(ws), wsb,
                                            stream_handle(DEV)))
    _untouched(out)
    idx = T(np.array([0, 1, 1, 3, 0, 2], np.int32))
    bag = T(np.array([0, 0, 1, 2, 4, 5], np.int32))
    wsb = lib().dr_segment_grad_workspace_size(n, n, U)
    ws = workspace(wsb, DEV)
    with pytest.raises(dr.DeepRecError):
        check(lib().dr_sparse_segment_reduce_grad(ptr(data), n, dim, ptr(idx), ptr(bag), n, U, 1,
                                                  ptr(out), ptr(ws), wsb, stream_handle(DEV)))
    _untouched(out)
    finish(dr)


def _grad_descs(_lib, grad, dim, seg, off, idx, num_unique):
    descs = (_lib.DrPoolGradDesc * 1)()
    d = descs[0]
    d.top_grad, d.top_stride = grad.data_ptr(), dim
    d.bag_off, d.seg, d.seg_stride = off.data_ptr(), seg.data_ptr(), 1
    d.idx = None if idx is None else idx.data_ptr()
    d.nnz = seg.numel()
    d.num_unique = None if num_unique is None else num_unique.data_ptr()
    d.combiner = 0
    return descs


@pytest.mark.parametrize("dim", [1028, 257])
def test_grouped_unique_backward_refuses_the_next_width(dr, dim):
    from deeprec_amd import _lib
    from deeprec_amd._lib import check, lib, ptr, stream_handle, workspace
    assert S.grad_class(dim) is None
    B, n = 3, 4
    grad = torch.ones((B, dim), device=DEV)
    seg = T(np.array([0, 1, 1, 2], np.int64))
    off = T(np.array([0, 1, 3, 4], np.int32))
    idx = T(np.array([0, 1, 0, 2], np.int32))
    nu = T(np.array([3], np.int64))
    gu = torch.full((n, dim), SENTINEL, device=DEV)
    descs = _grad_descs(_lib, grad, dim, seg, off, idx, nu)
    wsb = lib().dr_pool_grad_grouped_workspace_size(n)
    ws = workspace(wsb, DEV)
    with pytest.raises(dr.DeepRecError):
        check(lib().dr_pool_grad_grouped(descs, 1, B, dim, ptr(gu), ptr(ws), wsb,
                                         stream_handle(DEV)))
    _untouched(gu)
    finish(dr)


@pytest.mark.parametrize("dim", [1028, 1025])
def test_rows_backward_refuses_the_next_width(dr, dim):
    """kRowsMaxDim: refused before anything is launched."""
    from deeprec_amd import _lib
    from deeprec_amd._lib import check, lib, ptr, stream_handle, workspace
    assert S.rows_class(dim) is None
    B, n = 3, 4
    grad = torch.ones((B, dim), device=DEV)
    seg = T(np.array([0, 1, 1, 2], np.int64))
    off = T(np.array([0, 1, 3, 4], np.int32))
    rowsel = T(np.array([0, 1, 0, 2], np.int64))
    keys = T(np.array([5, 6, 5, 7], np.int64))
    uniq = torch.full((n,), -3, device=DEV, dtype=torch.int64)
    urows, gptr = torch.zeros_like(uniq), torch.zeros_like(uniq)
    nu = torch.zeros(1, device=DEV, dtype=torch.int64)
    gu = torch.full((n, dim), SENTINEL, device=DEV)
    descs = _grad_descs(_lib, grad, dim, seg, off, None, None)
    wsb = lib().dr_pool_grad_rows_workspace_size(n)
    ws = workspace(wsb, DEV)
    with pytest.raises(dr.DeepRecError):
        check(lib().dr_pool_grad_rows_grouped_ex2(descs, 1, B, dim, ptr(rowsel), 0, 8, ptr(keys),
                                                  0, ptr(uniq), ptr(urows), ptr(nu), ptr(gptr),
                                                  ptr(gu), ptr(ws), wsb, stream_handle(DEV)))
    _untouched(gu)
    assert bool((uniq == -3).all())
    finish(dr)


@pytest.mark.parametrize("dim,aligned", [(1028, True), (257, True), (260, False)])
def test_gather_refuses_the_next_width(dr, dim, aligned):
    """Past 1024, past 256 unaligned -- and 260 on a table that is not
    16-byte aligned, which the scalar classes (up to 256) do not cover."""
    from deeprec_amd._lib import check, lib, ptr, stream_handle
    assert S.gather_class(dim, aligned) is None
    buf = torch.zeros(8 * dim + 4, device=DEV)
    table = buf[0 if aligned else 1:][:8 * dim].view(8, dim)
    ids = torch.arange(5, device=DEV)
    out = torch.full((5, dim), SENTINEL, device=DEV)
    with pytest.raises(dr.DeepRecError):
        check(lib().dr_gather(ptr(table), 8, dim, ptr(ids), 5, ptr(out), stream_handle(DEV)))
    _untouched(out)
    finish(dr)


@pytest.mark.parametrize("dim", [1028, 1025])
def test_clip_by_norm_grad_refuses_the_next_width(dr, ops, dim):
    assert S.clip_grad_class(dim) is None
    pool = torch.ones((8, dim), device=DEV)
    g = torch.full((5, dim), SENTINEL, device=DEV)
    with pytest.raises(dr.DeepRecError):
        ops.clip_by_norm_grad(g, pool, torch.arange(5, device=DEV), 1.0, pool_rows=8)
    _untouched(g)
    finish(dr)
