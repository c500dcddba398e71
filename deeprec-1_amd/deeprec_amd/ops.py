"""Functional GPU ops with DeepRec/TF op names, on torch device tensors.

Each op calls the HIP C ABI (include/deeprec_amd.h) on torch's current stream.
Data-dependent errors (OP_REQUIRES in the reference) are latched on the
device; call `status_check()` or enable `set_validate(True)` to have every op
synchronise and raise, which is what the parity tests do.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import COMBINERS, ORDER_ALI, ORDER_SEQ, check, lib, ptr, stream_handle, workspace

_VALIDATE = os.environ.get("DEEPREC_AMD_VALIDATE", "0") == "1"


def set_validate(on):
    global _VALIDATE
    _VALIDATE = bool(on)


def _post(device):
    # (no validation sync while a hipGraph is being captured: the status word
    # is checked after the replay instead)
    if _VALIDATE and not torch.cuda.is_current_stream_capturing():
        _lib.status_check(device)


def status_check(device=None):
    _lib.status_check(device)


def _dev(t):
    if not t.is_cuda:
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT,
                                "deeprec_amd ops take device tensors (got %s)" % t.device)
    return t.device


def _c(t, dtype):
    return t.to(dtype).contiguous()


def _inner(t):
    """Elements per row of a [n, ...] tensor (also when n == 0)."""
    k = 1
    for x in t.shape[1:]:
        k *= int(x)
    return k


# ---------------------------------------------------------------------------
# Unique (UniqueAliOp, core/kernels/unique_ali_op.cc:46-180)
# ---------------------------------------------------------------------------
def unique_device(x, with_counts=False):
    """First-occurrence unique with NO host sync.

    Returns (y [n], idx [n] int32, counts [n] int32 or None, num_unique int64[1]);
    only y[:num_unique] / counts[:num_unique] are meaningful."""
    dev = _dev(x)
    i32 = x.dtype == torch.int32               # the int32 registration: y stays int32
    x = _c(x.reshape(-1), torch.int32 if i32 else torch.int64)
    n = x.numel()
    y = torch.empty(n, dtype=x.dtype, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev) if with_counts else None
    u = torch.empty(1, dtype=torch.int64, device=dev)
    if i32:
        wsb = lib().dr_unique_i32_workspace_size(n)
        ws = workspace(wsb, dev)
        check(lib().dr_unique_i32(ptr(x), n, ptr(y), ptr(idx), ptr(cnt), ptr(u), ptr(ws), wsb,
                                  stream_handle(dev)))
    else:
        wsb = lib().dr_unique_workspace_size(n)
        ws = workspace(wsb, dev)
        check(lib().dr_unique(ptr(x), n, ptr(y), ptr(idx), ptr(cnt), ptr(u), ptr(ws), wsb,
                              stream_handle(dev)))
    _post(dev)
    return y, idx, cnt, u


def _koff_array(koff):
    import ctypes as C
    return (C.c_int64 * len(koff))(*[int(k) for k in koff])


def unique_grouped(keys, koff, with_counts=False):
    """Grouped first-occurrence unique of T features in one pass.

    keys: concatenated [sum n_t] int64; koff: host offsets (T+1).  Returns
    (uniq, idx, counts or None, num_unique[T] int64 device); feature t's
    uniques are uniq[koff[t] : koff[t] + num_unique[t]], idx is feature-local."""
    dev = _dev(keys)
    k = _c(keys, torch.int64)
    n = k.numel()
    T = len(koff) - 1
    ka = _koff_array(koff)
    y = torch.empty(n, dtype=torch.int64, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev) if with_counts else None
    u = torch.empty(T, dtype=torch.int64, device=dev)
    wsb = lib().dr_unique_grouped_workspace_size(ka, T)
    ws = workspace(wsb, dev)
    check(lib().dr_unique_grouped(ptr(k), ka, T, ptr(y), ptr(idx), ptr(cnt), ptr(u), ptr(ws), wsb,
                                  stream_handle(dev)))
    _post(dev)
    return y, idx, cnt, u


def route_by_owner(uniq, koff, num_unique, world):
    """(owner, feature)-blocked send order of a grouped unique: returns
    (keys_send, tags_send, perm, counts[world, T]) with only the first
    counts.sum() entries meaningful."""
    dev = _dev(uniq)
    n = uniq.numel()
    T = len(koff) - 1
    ka = _koff_array(koff)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    tags = torch.empty(n, dtype=torch.int32, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty((world, T), dtype=torch.int64, device=dev)
    wsb = lib().dr_route_workspace_size(n, world, T)
    ws = workspace(wsb, dev)
    check(lib().dr_route_by_owner(ptr(uniq), ka, T, ptr(num_unique), world, ptr(keys), ptr(tags),
                                  ptr(perm), ptr(counts), ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    return keys, tags, perm, counts


def unique(x, out_idx=torch.int32):
    """tf.unique: (y, idx), y in first-occurrence order (syncs for |y|)."""
    y, idx, _, u = unique_device(x)
    k = int(u.item())
    return y[:k], idx.to(out_idx)


def unique_with_counts(x, out_idx=torch.int32):
    y, idx, cnt, u = unique_device(x, with_counts=True)
    k = int(u.item())
    return y[:k], idx.to(out_idx), cnt[:k]


# ---------------------------------------------------------------------------
# Gather / segment reductions
# ---------------------------------------------------------------------------
def gather(params, indices):
    """ResourceGather on a dense [R, D] table (gather_functor.h:36-115)."""
    dev = _dev(params)
    params = _c(params, torch.float32)
    idx = _c(indices.reshape(-1), torch.int64)
    D = params.shape[1]
    out = torch.empty((idx.numel(), D), dtype=torch.float32, device=dev)
    check(lib().dr_gather(ptr(params), params.shape[0], D, ptr(idx), idx.numel(), ptr(out),
                          stream_handle(dev)))
    _post(dev)
    return out.reshape(tuple(indices.shape) + (D,))


def _segment_reduce(data, indices, segment_ids, num_segments, combiner):
    dev = _dev(data)
    data = _c(data, torch.float32)
    data2 = data.reshape(data.shape[0], _inner(data))
    idx = _c(indices, torch.int32)
    seg = _c(segment_ids, torch.int32)
    if num_segments is None:  # output rows = last segment id + 1 (reference CPU)
        num_segments = int(seg[-1].item()) + 1 if seg.numel() else 0
    D = data2.shape[1]
    out = torch.empty((num_segments, D), dtype=torch.float32, device=dev)
    wsb = lib().dr_segment_workspace_size(num_segments)
    ws = workspace(wsb, dev)
    check(lib().dr_sparse_segment_reduce(ptr(data2), data2.shape[0], D, ptr(idx), ptr(seg),
                                         idx.numel(), num_segments, COMBINERS[combiner], ptr(out),
                                         ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    return out.reshape((num_segments,) + tuple(data.shape[1:]))


def sparse_segment_sum(data, indices, segment_ids, num_segments=None):
    return _segment_reduce(data, indices, segment_ids, num_segments, "sum")


def sparse_segment_mean(data, indices, segment_ids, num_segments=None):
    return _segment_reduce(data, indices, segment_ids, num_segments, "mean")


def sparse_segment_sqrt_n(data, indices, segment_ids, num_segments=None):
    return _segment_reduce(data, indices, segment_ids, num_segments, "sqrtn")


def _segment_grad(grad, indices, segment_ids, output_dim0, combiner):
    dev = _dev(grad)
    grad = _c(grad, torch.float32)
    g2 = grad.reshape(grad.shape[0], _inner(grad))
    idx = _c(indices, torch.int32)
    seg = _c(segment_ids, torch.int32)
    D = g2.shape[1]
    out = torch.empty((output_dim0, D), dtype=torch.float32, device=dev)
    wsb = lib().dr_segment_grad_workspace_size(idx.numel(), g2.shape[0], output_dim0)
    ws = workspace(wsb, dev)
    check(lib().dr_sparse_segment_reduce_grad(ptr(g2), g2.shape[0], D, ptr(idx), ptr(seg),
                                              idx.numel(), output_dim0, COMBINERS[combiner],
                                              ptr(out), ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    return out.reshape((output_dim0,) + tuple(grad.shape[1:]))


def sparse_segment_sum_grad(grad, indices, segment_ids, output_dim0):
    """Grad of SparseSegmentSum = unsorted_segment_sum(gather(grad, seg), idx, dim0)
    (math_grad.py:321-327), deterministic CPU order."""
    return _segment_grad(grad, indices, segment_ids, output_dim0, "sum")


def sparse_segment_mean_grad(grad, indices, segment_ids, output_dim0):
    return _segment_grad(grad, indices, segment_ids, output_dim0, "mean")


def sparse_segment_sqrt_n_grad(grad, indices, segment_ids, output_dim0):
    return _segment_grad(grad, indices, segment_ids, output_dim0, "sqrtn")


def unsorted_segment_sum(data, segment_ids, num_segments):
    """UnsortedSegmentSum (segment_reduction_ops.cc:377-405): serial order, seg<0 skipped."""
    dev = _dev(data)
    data = _c(data, torch.float32)
    d2 = data.reshape(data.shape[0], _inner(data))
    seg = _c(segment_ids, torch.int32)
    D = d2.shape[1]
    out = torch.empty((num_segments, D), dtype=torch.float32, device=dev)
    wsb = lib().dr_unsorted_segment_sum_workspace_size(seg.numel(), num_segments)
    ws = workspace(wsb, dev)
    check(lib().dr_unsorted_segment_sum(ptr(d2), d2.shape[0], D, ptr(seg), num_segments, ptr(out),
                                        ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    return out.reshape((num_segments,) + tuple(data.shape[1:]))


def bag_offsets(segment_ids, batch):
    """CSR offsets [batch+1] of sorted segment ids (int32 or int64)."""
    dev = _dev(segment_ids)
    off = torch.empty(batch + 1, dtype=torch.int32, device=dev)
    if segment_ids.dtype == torch.int32:
        s = segment_ids.contiguous()
        check(lib().dr_bag_offsets_i32(ptr(s), s.numel(), batch, ptr(off), stream_handle(dev)))
    else:
        s = _c(segment_ids, torch.int64)
        check(lib().dr_bag_offsets(ptr(s), s.numel(), batch, ptr(off), stream_handle(dev)))
    _post(dev)
    return off


def pool_grouped(descs, batch, dim, order=ORDER_ALI, device=None, onehot=False, bf16=False,
                 out_bf16=False):
    """Launch dr_pool_grouped_ex on a list of _lib.DrPoolDesc (<= 32 tables).
    onehot: every bag b holds exactly nnz b (bag_off not read).  bf16: the
    tables hold bf16 values (DR_POOL_BF16), pooled into fp32 -- or into bf16
    with out_bf16 (DR_POOL_OUT_BF16); strides in elements of their type."""
    arr = (_lib.DrPoolDesc * len(descs))(*descs)
    flags = ((_lib.POOL_ONEHOT if onehot else 0) | (_lib.POOL_BF16 if bf16 else 0)
             | (_lib.POOL_OUT_BF16 if out_bf16 else 0))
    check(lib().dr_pool_grouped_ex(arr, len(descs), batch, dim, order, flags,
                                   stream_handle(device)))
    _post(device)


def sort_pairs(keys, vals, bit_hi, bit_lo=0):
    """Stable LSD radix sort of (uint64 key, int32 value) pairs."""
    dev = _dev(keys)
    k = _c(keys, torch.int64)
    v = _c(vals, torch.int32)
    ko = torch.empty_like(k)
    vo = torch.empty_like(v)
    wsb = lib().dr_sort_pairs_workspace_size(k.numel())
    ws = workspace(wsb, dev)
    check(lib().dr_sort_pairs(ptr(k), ptr(v), ptr(ko), ptr(vo), k.numel(), bit_lo, bit_hi, ptr(ws),
                              wsb, stream_handle(dev)))
    _post(dev)
    return ko, vo


# ---------------------------------------------------------------------------
# embedding_lookup_sparse / safe_embedding_lookup_sparse through the single
# C entry dr_embedding_lookup_sparse (embedding_ops.py:480-675, :1209-1344):
# what a TF custom-op kernel binds.  Forward only.
# ---------------------------------------------------------------------------
def embedding_lookup_sparse_c(params, sp_indices, sp_values, batch, sp_weights=None,
                              combiner="mean", max_norm=None, safe=False, default_id=None,
                              prune=True, read_only=False):
    """params: an EmbeddingVariable (handle / dim attributes) or a dense fp32
    [rows, dim] tensor.  sp_indices [nnz, 2] int64 rows-sorted, sp_values
    [nnz] int64, sp_weights [nnz] fp32 or None.  Returns [batch, dim].
    read_only: dr_embedding_lookup_sparse_readonly (an EV, left unchanged)."""
    ind = sp_indices.to(torch.int64).contiguous()
    val = sp_values.to(torch.int64).contiguous()
    w = None if sp_weights is None else sp_weights.to(torch.float32).contiguous()
    nnz = val.numel()
    dev = val.device
    if torch.is_tensor(params):
        ev, table = None, params.contiguous()
        rows, dim = table.shape
    else:
        ev, table, rows, dim = params.handle, None, 0, params.dim
    out = torch.empty((batch, dim), dtype=torch.float32, device=dev)
    entry = "dr_embedding_lookup_sparse_readonly" if read_only else "dr_embedding_lookup_sparse"
    wsb = getattr(lib(), entry + "_workspace_size")(nnz, batch)
    ws = workspace(wsb, dev)
    check(getattr(lib(), entry)(
        ev, ptr(table), rows, dim, ptr(ind), ptr(val), ptr(w), nnz, batch, COMBINERS[combiner],
        -1.0 if max_norm is None else float(max_norm), 1 if safe else 0,
        -1 if default_id is None else int(default_id), 1 if prune else 0, ptr(out), dim,
        ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    return out


# ---------------------------------------------------------------------------
# Fused embedding ops (core/ops/fused_embedding_ops.cc:12-58)
# ---------------------------------------------------------------------------
def fused_embedding_local_sparse_look_up(sp_values, sp_indices, sp_dense_shape, emb_variable,
                                         combiner="mean", max_norm=-1.0):
    dev = _dev(emb_variable)
    table = _c(emb_variable, torch.float32)
    vals = _c(sp_values, torch.int64)
    ind = _c(sp_indices, torch.int64)
    B = int(sp_dense_shape[0])
    D = table.shape[1]
    out = torch.empty((B, D), dtype=torch.float32, device=dev)
    vo = torch.empty(B, dtype=torch.int32, device=dev)
    wsb = lib().dr_fused_local_workspace_size(B)
    ws = workspace(wsb, dev)
    check(lib().dr_fused_local_lookup(ptr(table), table.shape[0], D, ptr(vals), ptr(ind),
                                      vals.numel(), B, COMBINERS[combiner], float(max_norm),
                                      ptr(out), ptr(vo), ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    return out, vo


def fused_embedding_local_sparse_look_up_grad(top_grad, emb_variable, sp_values,
                                              sp_values_offset, combiner="mean", max_norm=-1.0):
    dev = _dev(top_grad)
    tg = _c(top_grad, torch.float32)
    table = _c(emb_variable, torch.float32)
    vals = _c(sp_values, torch.int64)
    vo = _c(sp_values_offset, torch.int32)
    D = tg.shape[1]
    out = torch.empty((vals.numel(), D), dtype=torch.float32, device=dev)
    check(lib().dr_fused_local_lookup_grad(ptr(tg), ptr(table), table.shape[0], D, ptr(vals),
                                           ptr(vo), vals.numel(), tg.shape[0],
                                           COMBINERS[combiner], float(max_norm), ptr(out),
                                           stream_handle(dev)))
    _post(dev)
    return out


def _combiner(combiner):
    if combiner not in COMBINERS:
        raise ValueError("combiner must be one of 'mean', 'sqrtn' or 'sum'")
    return COMBINERS[combiner]


def _max_norm(max_norm):
    return -1.0 if max_norm is None else float(max_norm)


def fused_embedding_sparse_pre_look_up(partition_shapes, sp_values, sp_indices):
    """FusedEmbeddingSparsePreLookUp (core/ops/fused_embedding_ops.cc:60-107,
    fused_embedding_ops_gpus.cu.cc:150-283): ids stably sorted and split by
    the "div" boundaries of partition_shapes[i][0], rebased per partition.
    Returns (partitioned_values, partitioned_indices) lists.  Like the
    reference kernel (:228-238) it reads the partition sizes back to the host
    once to shape its outputs."""
    dev = _dev(sp_values)
    rows = [int(s[0]) for s in partition_shapes]
    P = len(rows)
    if P < 1 or P > _lib.MAX_PARTITIONS:
        raise ValueError("num_partitions must be in [1, %d]" % _lib.MAX_PARTITIONS)
    vals = _c(sp_values.reshape(-1), torch.int64)
    ind = _c(sp_indices, torch.int64)
    n = vals.numel()
    if ind.shape != (n, 2):
        raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, "sp_indices must be [nnz, 2]")
    import ctypes as C
    vout = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    iout = torch.empty((max(n, 1), 2), dtype=torch.int64, device=dev)
    off = torch.empty(P + 1, dtype=torch.int64, device=dev)
    wsb = lib().dr_fused_pre_lookup_workspace_size(n)
    ws = workspace(wsb, dev)
    check(lib().dr_fused_pre_lookup(ptr(vals), ptr(ind), n, (C.c_int64 * P)(*rows), P, ptr(vout),
                                    ptr(iout), ptr(off), ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    o = off.cpu().tolist()
    return ([vout[o[p]:o[p + 1]] for p in range(P)], [iout[o[p]:o[p + 1]] for p in range(P)])


def _shard_arrays(emb_shards, partitioned_indices):
    import ctypes as C
    P = len(emb_shards)
    if P < 1 or P > _lib.MAX_PARTITIONS or len(partitioned_indices) != P:
        raise ValueError("need 1..%d emb_shards with one partitioned_indices each"
                         % _lib.MAX_PARTITIONS)
    shards = [_c(s, torch.float32) for s in emb_shards]
    inds = [_c(i, torch.int64) for i in partitioned_indices]
    for s, i in zip(shards, inds):
        if s.shape[0] != i.shape[0]:
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "emb_shard and partitioned_indice dosn't have the same length")
    A = C.c_void_p * P
    sp = A(*[s.data_ptr() if s.numel() else None for s in shards])
    ip = A(*[i.data_ptr() if i.numel() else None for i in inds])
    rows = (C.c_int64 * P)(*[s.shape[0] for s in shards])
    return shards, inds, sp, ip, rows


def fused_embedding_sparse_post_look_up(emb_shards, partitioned_indices, sp_dense_shape,
                                        partitioned_values=None, combiner="mean", max_norm=None):
    """FusedEmbeddingSparsePostLookUp (core/ops/fused_embedding_ops.cc:109-155,
    fused_embedding_ops_gpus.cu.cc:285-384) -> (emb_vectors [B, D],
    feature_nums [B] int32).  Bags are summed in (row, col) order, so the
    result equals the local fused lookup of the same ids bit for bit."""
    dev = _dev(emb_shards[0])
    shards, inds, sp, ip, rows = _shard_arrays(emb_shards, partitioned_indices)
    P = len(shards)
    D = shards[0].shape[1]
    B, cols = int(sp_dense_shape[0]), int(sp_dense_shape[1])
    out = torch.empty((B, D), dtype=torch.float32, device=dev)
    fnum = torch.empty(B, dtype=torch.int32, device=dev)
    N = sum(s.shape[0] for s in shards)
    wsb = lib().dr_fused_post_lookup_workspace_size(N, B)
    ws = workspace(wsb, dev)
    check(lib().dr_fused_post_lookup(sp, ip, rows, P, B, max(cols, 1), D, _combiner(combiner),
                                     _max_norm(max_norm), ptr(out), ptr(fnum), ptr(ws), wsb,
                                     stream_handle(dev)))
    _post(dev)
    return out, fnum


def fused_embedding_sparse_post_look_up_grad(top_grad, emb_shards, partitioned_indices,
                                             feature_nums, combiner="mean", max_norm=None):
    """FusedEmbeddingSparsePostLookUpGrad (core/ops/fused_embedding_ops.cc:157-196,
    fused_embedding_ops_gpus.cu.cc:386-514) -> grad_shards list."""
    import ctypes as C
    dev = _dev(top_grad)
    tg = _c(top_grad, torch.float32)
    shards, inds, sp, ip, rows = _shard_arrays(emb_shards, partitioned_indices)
    P = len(shards)
    D = tg.shape[1]
    outs = [torch.empty((s.shape[0], D), dtype=torch.float32, device=dev) for s in shards]
    fn = _c(feature_nums, torch.int32)
    check(lib().dr_fused_post_lookup_grad(
        ptr(tg), sp, ip, rows, P, tg.shape[0], D, ptr(fn), _combiner(combiner),
        _max_norm(max_norm), (C.c_void_p * P)(*[o.data_ptr() if o.numel() else None
                                               for o in outs]), stream_handle(dev)))
    _post(dev)
    return outs


def bag_weight_scale(weights, bag_off, combiner):
    """Per-bag divisor of a weighted lookup: sum(w) (mean) / sqrt(sum(w^2))."""
    dev = _dev(weights)
    B = bag_off.numel() - 1
    q = torch.empty(max(B, 1), dtype=torch.float32, device=dev)
    check(lib().dr_bag_weight_scale(ptr(weights), ptr(bag_off), B, _combiner(combiner), ptr(q),
                                    stream_handle(dev)))
    _post(dev)
    return q


def clip_by_norm_grad(grad, pool, rows, max_norm, pool_rows=None, default_rows=None,
                      default_stride=0, n_dev=None):
    """In place: grad [n, D] of clip_by_norm(pool[rows], max_norm) -> grad of
    the unclipped rows (clip_ops.py:164-184 chain rule)."""
    dev = _dev(grad)
    n, D = grad.shape
    pr = (1 << 62) if pool_rows is None else int(pool_rows)
    dr_ = default_rows if isinstance(default_rows, int) else ptr(default_rows)
    check(lib().dr_clip_by_norm_grad(pool if isinstance(pool, int) else ptr(pool), pr, ptr(rows),
                                     dr_, int(default_stride), ptr(n_dev), n, D,
                                     float(max_norm), ptr(grad), stream_handle(dev)))
    _post(dev)
    return grad


# ---------------------------------------------------------------------------
# Interactions
# ---------------------------------------------------------------------------
def fm_second_order(emb):
    """0.5 * ((sum_f e)^2 - sum_f e^2) over [B, F, D] (DeepFM train.py:205-209)."""
    dev = _dev(emb)
    e = _c(emb, torch.float32)
    B, F, D = e.shape
    out = torch.empty((B, D), dtype=torch.float32, device=dev)
    check(lib().dr_fm2(ptr(e), B, F, D, ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def fm_second_order_grad(emb, top_grad):
    dev = _dev(emb)
    e = _c(emb, torch.float32)
    g = _c(top_grad, torch.float32)
    B, F, D = e.shape
    out = torch.empty_like(e)
    check(lib().dr_fm2_grad(ptr(e), ptr(g), B, F, D, ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def fm_second_order_bf16_copy(emb):
    """dr_fm2_bf16_copy: (fm [B, D] fp32, bf16 copy of emb as [B, F*D])."""
    dev = _dev(emb)
    emb = _c(emb, torch.float32)
    B, F, D = emb.shape
    out = torch.empty((B, D), dtype=torch.float32, device=dev)
    cp = torch.empty((B, F * D), dtype=torch.bfloat16, device=dev)
    check(lib().dr_fm2_bf16_copy(ptr(emb), B, F, D, ptr(out), ptr(cp), stream_handle(dev)))
    _post(dev)
    return out, cp


def fm_second_order_grad_add_bf16(emb, top_grad, add):
    """dr_fm2_grad_add_bf16: FM gradient + float(add) (add bf16 [B, F*D])."""
    dev = _dev(emb)
    emb = _c(emb, torch.float32)
    g = _c(top_grad, torch.float32)
    B, F, D = emb.shape
    if add.dtype != torch.bfloat16 or add.stride(1) != 1:
        raise ValueError("add must be bf16 with unit column stride")
    out = torch.empty_like(emb)
    check(lib().dr_fm2_grad_add_bf16(ptr(emb), ptr(g), ptr(add), add.stride(0), B, F, D, ptr(out),
                                     stream_handle(dev)))
    _post(dev)
    return out


def dot_interaction(x):
    """DLRM dot_op (DLRM train.py:150-163): strictly-lower triangle of X X^T."""
    dev = _dev(x)
    x = _c(x, torch.float32)
    B, F, D = x.shape
    out = torch.empty((B, F * (F - 1) // 2), dtype=torch.float32, device=dev)
    check(lib().dr_dot_interaction(ptr(x), B, F, D, ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def dot_interaction_grad(x, top_grad):
    """Backward of dot_interaction: [B, F, D] grad of X."""
    dev = _dev(x)
    x = _c(x, torch.float32)
    g = _c(top_grad, torch.float32)
    B, F, D = x.shape
    out = torch.empty_like(x)
    check(lib().dr_dot_interaction_grad(ptr(x), ptr(g), B, F, D, ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def dot_interaction_concat_bf16(x, out_cols):
    """DLRM dot layer + concat + --bf16 cast (modelzoo/DLRM/train.py:211-226):
    x [B, F, D] fp32 with x[:, 0] = dense_inputs -> bf16 [B, out_cols] =
    x[:, 0] | dot_interaction(x) | zero padding (dr_dot_interaction_concat_bf16)."""
    dev = _dev(x)
    x = _c(x, torch.float32)
    B, F, D = x.shape
    out = torch.empty((B, out_cols), dtype=torch.bfloat16, device=dev)
    check(lib().dr_dot_interaction_concat_bf16(ptr(x), B, F, D, ptr(out), out_cols,
                                               stream_handle(dev)))
    _post(dev)
    return out


def dot_interaction_concat_grad_bf16(x, grad):
    """Backward of dot_interaction_concat_bf16 from the bf16 [B, cols] gradient."""
    dev = _dev(x)
    x = _c(x, torch.float32)
    if grad.dtype != torch.bfloat16 or grad.stride(1) != 1:
        raise ValueError("grad must be bf16 with unit column stride")
    B, F, D = x.shape
    out = torch.empty_like(x)
    check(lib().dr_dot_interaction_concat_grad_bf16(ptr(x), ptr(grad), grad.stride(0), B, F, D,
                                                    ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def relu_grad_bf16(g, y):
    """dr_relu_grad_bf16: bf16(g) masked by y > 0 (y the bf16 ReLU output);
    g fp32 [R, C] with unit column stride (any row stride)."""
    dev = _dev(g)
    R, C = y.shape
    if g.dtype != torch.float32 or g.stride(1) != 1 or y.dtype != torch.bfloat16 \
            or y.stride(1) != 1 or tuple(g.shape) != (R, C):
        raise ValueError("relu_grad_bf16 needs fp32 g and bf16 y of one shape, unit column stride")
    out = torch.empty((R, C), dtype=torch.bfloat16, device=dev)
    check(lib().dr_relu_grad_bf16(ptr(g), g.stride(0), ptr(y), y.stride(0), R, C, ptr(out), C,
                                  stream_handle(dev)))
    _post(dev)
    return out


def mlp_head_forward(h, w, bias=None):
    """dr_mlp_head_forward_bf16: the N = 1 output layer on the bf16 tower
    output h [B, K] -> z [B] fp32.  w bf16: the bf16 layer (a bf16-rounded
    logit); w fp32: the fp32 layer on the widened h.  bias a 1-element fp32
    device tensor or None."""
    dev = _dev(h)
    B, K = h.shape
    if h.dtype != torch.bfloat16 or h.stride(1) != 1 or \
            w.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("mlp_head_forward needs bf16 h (unit column stride), bf16 / fp32 w")
    z = torch.empty(B, dtype=torch.float32, device=dev)
    bb = None if bias is None else _c(bias.reshape(1), torch.float32)
    check(lib().dr_mlp_head_forward_bf16(ptr(h), h.stride(0), B, K, ptr(w.contiguous()),
                                         1 if w.dtype == torch.float32 else 0, ptr(bb), ptr(z),
                                         stream_handle(dev)))
    _post(dev)
    return z


def mlp_head_backward(h, w, gz):
    """dr_mlp_head_backward_bf16 -> (grad_h bf16 [B, K] with h's ReLU mask
    applied, dw fp32 [K], db fp32 scalar tensor); w as in mlp_head_forward."""
    dev = _dev(h)
    B, K = h.shape
    gz = _c(gz.reshape(B), torch.float32)
    P = lib().dr_mlp_head_grad_partials(B)
    gh = torch.empty((B, K), dtype=torch.bfloat16, device=dev)
    dwp = torch.empty((max(P, 1), K), dtype=torch.float32, device=dev)
    dbp = torch.empty(max(P, 1), dtype=torch.float32, device=dev)
    check(lib().dr_mlp_head_backward_bf16(ptr(h), h.stride(0), B, K, ptr(w.contiguous()),
                                          1 if w.dtype == torch.float32 else 0, ptr(gz), ptr(gh),
                                          K, ptr(dwp), ptr(dbp), stream_handle(dev)))
    _post(dev)
    return gh, dwp[:P].sum(0), dbp[:P].sum()


def crossnet_layer(x0, xl, weight, bias=None):
    """DCN-v2 cross layer x0 * (xl W^T + b) + xl, bf16 MFMA, fp32 accumulate.

    Feature dims that are not a multiple of 64 are zero-padded (exact); a
    caller that keeps its features padded (modelzoo.DCNv2) pays no copy."""
    dev = _dev(x0)
    B, d = x0.shape
    dp = (d + 63) // 64 * 64

    def pad2(t, rows, cols):
        t = t.to(torch.bfloat16)
        if t.shape[1] == cols and t.shape[0] == rows:
            return t.contiguous()
        o = torch.zeros((rows, cols), dtype=torch.bfloat16, device=dev)
        o[:t.shape[0], :t.shape[1]] = t
        return o

    a0 = pad2(x0, B, dp)
    al = pad2(xl, B, dp)
    w = pad2(weight, dp, dp)
    b = None
    if bias is not None:
        b = torch.zeros(dp, dtype=torch.float32, device=dev)
        b[:d] = bias.float()
    out, _ = crossnet_forward(a0, al, w, b, with_lin=False)
    return out[:, :d]


def crossnet_forward(x0, xl, weight, bias, with_lin=True):
    """dr_crossnet_forward_bf16 on padded operands: x0 / xl [B, d] bf16,
    weight [d, d] bf16 (out, in), bias [d] fp32 or None, d % 64 == 0.
    Returns (out [B, d] bf16, lin = xl W^T + b [B, d] bf16 or None)."""
    dev = _dev(x0)
    B, d = x0.shape
    if d % 64 or x0.dtype != torch.bfloat16 or xl.dtype != torch.bfloat16 \
            or weight.dtype != torch.bfloat16 or tuple(weight.shape) != (d, d):
        raise ValueError("crossnet_forward needs bf16 operands with d % 64 == 0")
    x0, xl, weight = x0.contiguous(), xl.contiguous(), weight.contiguous()
    b = None if bias is None else bias.to(torch.float32).contiguous()
    out = torch.empty((B, d), dtype=torch.bfloat16, device=dev)
    lin = torch.empty((B, d), dtype=torch.bfloat16, device=dev) if with_lin else None
    check(lib().dr_crossnet_forward_bf16(ptr(x0), ptr(xl), ptr(weight), ptr(b), B, d, ptr(out),
                                         ptr(lin), stream_handle(dev)))
    _post(dev)
    return out, lin


ACT_NONE, ACT_RELU, ACT_MASK = 0, 1, 2


def gemm_nt(a, b, bias=None, act=ACT_NONE, out_fp32=False, split_k=1, out=None, mask=None):
    """dr_gemm_nt_bf16[_ex]: act(a b^T + bias) with a [M, K], b [N, K] bf16
    (row strides free, unit column stride), K % 64 == 0, N % 8 == 0; fp32
    accumulate; bf16 (or fp32) [M, N] output.  split_k > 1: K cut into
    chunks summed in chunk order (deterministic).  mask (bf16 [M, N]): the
    result is zeroed where mask <= 0 (act ACT_MASK, a ReLU's backward)."""
    dev = _dev(a)
    M, K = a.shape
    N = b.shape[0]
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or b.shape[1] != K \
            or a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError("gemm_nt needs bf16 a [M, K], b [N, K] with unit column stride")
    odt = torch.float32 if out_fp32 else torch.bfloat16
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=dev)
    bb = None if bias is None else bias.to(torch.float32).contiguous()
    wsb = lib().dr_gemm_nt_workspace_size(M, N, split_k)
    ws = workspace(wsb, dev) if wsb else None
    if mask is not None:
        if mask.dtype != torch.bfloat16 or tuple(mask.shape) != (M, N) or mask.stride(1) != 1:
            raise ValueError("mask must be bf16 [M, N] with unit column stride")
        act = ACT_MASK
    check(lib().dr_gemm_nt_bf16_ex(ptr(a), a.stride(0), ptr(b), b.stride(0), M, N, K, ptr(bb), act,
                                   ptr(mask), mask.stride(0) if mask is not None else 0, ptr(out),
                                   out.stride(0), 1 if out_fp32 else 0, split_k, ptr(ws), wsb,
                                   stream_handle(dev)))
    _post(dev)
    return out


def gemm_tn(g, x, split_k=1, colsum=False):
    """dr_gemm_tn_bf16: g^T x in fp32 for g [R, N], x [R, K] bf16 (unit column
    strides, R % 64 == 0): [N, K]; colsum=True also returns g's fp32 column
    sums (the bias gradient): (dw, db)."""
    dev = _dev(g)
    R, N = g.shape
    K = x.shape[1]
    if g.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or x.shape[0] != R \
            or g.stride(1) != 1 or x.stride(1) != 1:
        raise ValueError("gemm_tn needs bf16 g [R, N], x [R, K] with unit column stride")
    out = torch.empty((N, K), dtype=torch.float32, device=dev)
    cs = torch.empty(N, dtype=torch.float32, device=dev) if colsum else None
    wsb = lib().dr_gemm_tn_workspace_size(N, K, split_k, 1 if colsum else 0)
    ws = workspace(wsb, dev) if wsb else None
    check(lib().dr_gemm_tn_bf16(ptr(g), g.stride(0), ptr(x), x.stride(0), R, N, K, ptr(out), K,
                                ptr(cs), split_k, ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    return (out, cs) if colsum else out


def transpose_bf16(x, colsum=False):
    """dr_transpose_bf16: [R, C] bf16 (unit column stride) -> contiguous [C, R].
    colsum=True (dr_transpose_bf16_colsum): also the fp32 column sums of x,
    from per-64-row-tile partials summed in tile order; returns (out, sums)."""
    dev = _dev(x)
    R, Cc = x.shape
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise ValueError("transpose_bf16 needs a bf16 matrix with unit column stride")
    out = torch.empty((Cc, R), dtype=torch.bfloat16, device=dev)
    if not colsum:
        check(lib().dr_transpose_bf16(ptr(x), R, Cc, x.stride(0), ptr(out), R,
                                      stream_handle(dev)))
        _post(dev)
        return out
    part = torch.empty(((R + 63) // 64, Cc), dtype=torch.float32, device=dev)
    check(lib().dr_transpose_bf16_colsum(ptr(x), R, Cc, x.stride(0), ptr(out), R, ptr(part),
                                         stream_handle(dev)))
    _post(dev)
    return out, part.sum(0)


def crossnet_dx(u, wt, g):
    """dr_crossnet_dx_bf16: dx = u W + g for a cross layer's input gradient,
    wt = W^T [d, d] bf16 contiguous; u, g [B, d] bf16, d % 64 == 0.  One
    rounding of the fp32 u W + g (torch.addmm(g, u, W) in bf16)."""
    dev = _dev(u)
    B, d = u.shape
    if d % 64 or tuple(g.shape) != (B, d) or tuple(wt.shape) != (d, d) or any(
            t.dtype != torch.bfloat16 for t in (u, wt, g)):
        raise ValueError("crossnet_dx needs bf16 u, g [B, d] and wt [d, d] with d % 64 == 0")
    u, wt, g = u.contiguous(), wt.contiguous(), g.contiguous()
    dx = torch.empty((B, d), dtype=torch.bfloat16, device=dev)
    check(lib().dr_crossnet_dx_bf16(ptr(u), ptr(wt), ptr(g), B, d, ptr(dx), stream_handle(dev)))
    _post(dev)
    return dx


def crossnet_dw(u, xl):
    """dr_crossnet_dw_bf16: dW = u^T x_l (fp32 [d, d]) for a cross layer's
    weight gradient; u, xl [B, d] bf16, d and B multiples of 64 (None
    otherwise: the caller falls back to a library GEMM)."""
    dev = _dev(u)
    B, d = u.shape
    if d % 64 or B % 64 or tuple(xl.shape) != (B, d) or any(
            t.dtype != torch.bfloat16 for t in (u, xl)):
        return None
    u, xl = u.contiguous(), xl.contiguous()
    dw = torch.empty((d, d), dtype=torch.float32, device=dev)
    wsb = lib().dr_crossnet_dw_workspace_size(B, d)
    ws = workspace(wsb, dev)
    check(lib().dr_crossnet_dw_bf16(ptr(u), ptr(xl), B, d, ptr(dw), ptr(ws), wsb,
                                    stream_handle(dev)))
    _post(dev)
    return dw


def crossnet_backward_elem(g, x0, lin, acc=None):
    """dr_crossnet_backward_elem_bf16: the elementwise part of a cross
    layer's backward in one pass.  g, x0, lin [B, d] bf16; acc [B, d] fp32
    running dx0 (None: start at 0; updated in place).  Returns (u = g * x0
    bf16, acc + g * lin fp32, db = column sums of u fp32)."""
    dev = _dev(g)
    B, d = g.shape
    for t in (g, x0, lin):
        if t.dtype != torch.bfloat16 or tuple(t.shape) != (B, d):
            raise ValueError("crossnet_backward_elem needs bf16 [B, d] operands")
    g, x0, lin = g.contiguous(), x0.contiguous(), lin.contiguous()
    out = torch.empty((B, d), dtype=torch.float32, device=dev) if acc is None else acc
    if acc is not None and (acc.dtype != torch.float32 or not acc.is_contiguous()
                            or tuple(acc.shape) != (B, d)):
        raise ValueError("acc must be a contiguous fp32 [B, d] tensor")
    u = torch.empty((B, d), dtype=torch.bfloat16, device=dev)
    db = torch.empty(d, dtype=torch.float32, device=dev)
    wsb = lib().dr_crossnet_backward_workspace_size(B, d)
    ws = workspace(wsb, dev)
    check(lib().dr_crossnet_backward_elem_bf16(ptr(g), ptr(x0), ptr(lin), ptr(acc), ptr(out),
                                               ptr(u), ptr(db), B, d, ptr(ws), wsb,
                                               stream_handle(dev)))
    _post(dev)
    return u, out, db


# ---------------------------------------------------------------------------
# DIN attention (modelzoo/DIN/script/utils.py:264-309, script/model.py:94-98)
# ---------------------------------------------------------------------------
def din_attention_input(query, facts):
    """din_all = concat([q, f, q - f, q * f], -1): query [B, H], facts
    [B, T, H] -> [B, T, 4H] (utils.py:280-282)."""
    dev = _dev(facts)
    B, T, H = facts.shape
    q, f = _c(query, torch.float32), _c(facts, torch.float32)
    out = torch.empty((B, T, 4 * H), dtype=torch.float32, device=dev)
    check(lib().dr_din_attention_input(ptr(q), ptr(f), B, T, H, ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def din_attention_input_grad(query, facts, top_grad, grad_facts=None):
    """Backward of din_attention_input -> (grad_query [B, H], grad_facts
    [B, T, H]); when grad_facts is given it is accumulated into in place."""
    dev = _dev(facts)
    B, T, H = facts.shape
    q, f, g = _c(query, torch.float32), _c(facts, torch.float32), _c(top_grad, torch.float32)
    gq = torch.empty((B, H), dtype=torch.float32, device=dev)
    acc = grad_facts is not None
    if not acc:
        grad_facts = torch.empty((B, T, H), dtype=torch.float32, device=dev)
    elif not grad_facts.is_contiguous() or grad_facts.dtype != torch.float32:
        raise ValueError("grad_facts must be a contiguous fp32 tensor")
    check(lib().dr_din_attention_input_grad(ptr(q), ptr(f), ptr(g), B, T, H, ptr(gq),
                                            ptr(grad_facts), int(acc), stream_handle(dev)))
    _post(dev)
    return gq, grad_facts


DIN_MLP_HIDDEN = (16, 32, 36, 64)


class DinMlpBuffers(object):
    """The fused DIN attention MLP's buffers (dr_din_mlp_buf) for one step:
    forward state kept for the backward, backward outputs the weight
    gradients are formed from.  cap = batch * seq_len (no host read of the
    valid-position count P).  The per-position buffers (h1t, h2t, da1t, da2t,
    xt, dsc) hold positions [0, P) only: with the hand weight-gradient pass
    their columns p >= P stay unwritten (uninitialised memory) and that pass
    stops at P itself; the library GEMM path asks the backward to zero the
    backward buffers' columns past P (zero_tail = 1).

    fill (test hook, None in use): a value every per-position buffer is
    filled with when allocated, so a test can show the hand pass never reads
    past P (NaN there must not reach a gradient)."""

    fill = None

    def __init__(self, B, T, H, n1, n2, dev):
        cap = B * T
        i32, f32 = torch.int32, torch.float32
        e = lambda shape, dt=f32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        self.pos, self.cnt, self.off = e(cap, i32), e(B, i32), e(B + 1, i32)
        self.w1p, self.w2t, self.cq = e((n1, 2 * H)), e((n1, n2)), e((B, n1))
        self.h1t, self.h2t = self._filled(e((n1, cap))), self._filled(e((n2, cap)))
        self.da1t = self.da2t = self.xt = self.dsc = self.dqp = self.s1 = self.dq2 = None
        self.B, self.T, self.H, self.n1, self.n2, self.cap = B, T, H, n1, n2, cap

    def _filled(self, t):
        return t if self.fill is None else t.fill_(self.fill)

    def alloc_backward(self, dev):
        B, H, n1, n2, cap = self.B, self.H, self.n1, self.n2, self.cap
        e = lambda shape: self._filled(torch.empty(shape, dtype=torch.float32, device=dev))  # noqa: E731
        self.da1t, self.da2t, self.xt = e((n1, cap)), e((n2, cap)), e((2 * H, cap))
        self.dsc, self.dqp, self.s1, self.dq2 = e(cap), e((H, cap)), e((B, n1)), e((B, H))

    def struct(self):
        names = [f[0] for f in _lib.DrDinMlpBuf._fields_]
        return _lib.DrDinMlpBuf(*[ptr(getattr(self, n)) for n in names])


def din_mlp_forward(query, facts, mask, w1, b1, w2, b2, w3, b3):
    """Fused attention MLP (dr_din_mlp_forward): scores [B, T] at the valid
    positions (the padded ones are 0 here and masked by the pool), and the
    buffers its backward needs."""
    dev = _dev(facts)
    B, T, H = facts.shape
    n1, n2 = w1.shape[0], w2.shape[0]
    q, f, m = _c(query, torch.float32), _c(facts, torch.float32), _c(mask, torch.float32)
    w1c, b1c, w2c, b2c = (_c(x, torch.float32) for x in (w1, b1, w2, b2))
    w3c, b3c = _c(w3.reshape(-1), torch.float32), _c(b3.reshape(-1), torch.float32)
    buf = DinMlpBuffers(B, T, H, n1, n2, dev)
    scores = torch.zeros((B, T), dtype=torch.float32, device=dev)
    st = buf.struct()
    check(lib().dr_din_mlp_forward(ptr(q), ptr(f), ptr(m), B, T, H, ptr(w1c), ptr(b1c), n1,
                                   ptr(w2c), ptr(b2c), n2, ptr(w3c), ptr(b3c), ptr(scores),
                                   C.byref(st), stream_handle(dev)))
    _post(dev)
    return scores, buf


# the attention MLP's weight gradients: one hand split-K pass on the matrix
# cores (dr_din_mlp_wgrad_valid over the valid positions, default: 0.085 + 0.008
# ms at DIN's configs[3])
# or, DR_DIN_WGRAD=lib, library GEMMs + reductions (≈ 0.25 ms;
# profiles/r05_din_wgrad.log)
_DIN_WGRAD_HAND = os.environ.get("DR_DIN_WGRAD", "hand") == "hand"


def din_mlp_backward(query, facts, w1, w3, buf, grad_scores, grad_facts):
    """Backward of din_mlp_forward: adds the MLP's part to grad_facts (in
    place) and returns (grad_query, dW1, db1, dW2, db2, dw3, db3); the weight
    gradients come from the feature-major per-position buffers: one hand pass
    bounded by the valid count, or library split-K GEMMs over cap (for which
    the backward zeroes the columns past the valid count)."""
    dev = _dev(facts)
    B, T, H = facts.shape
    n1, n2, cap = buf.n1, buf.n2, buf.cap
    q, f = _c(query, torch.float32), _c(facts, torch.float32)
    w3c = _c(w3.reshape(-1), torch.float32)
    gs = _c(grad_scores, torch.float32)
    if not grad_facts.is_contiguous() or grad_facts.dtype != torch.float32:
        raise ValueError("grad_facts must be a contiguous fp32 tensor")
    buf.alloc_backward(dev)
    st = buf.struct()
    hand = _DIN_WGRAD_HAND and 2 * H in (32, 64, 72, 128) and (n1, n2) == (80, 40) and cap % 4 == 0
    # the hand pass stops at the valid count P itself: the columns p >= P of
    # the per-position buffers stay unwritten (1.25 KB per position less)
    check(lib().dr_din_mlp_backward_tail(ptr(q), ptr(f), B, T, H, n1, n2, ptr(w3c), ptr(gs),
                                         ptr(grad_facts), C.byref(st), 0 if hand else 1,
                                         stream_handle(dev)))
    _post(dev)
    S = 64
    while S > 1 and cap % S:
        S //= 2
    L = cap // S

    def kred(a_t, b_t):   # a_t [M, cap], b_t [N, cap] -> a_t b_t^T, split over cap
        M, N = a_t.shape[0], b_t.shape[0]
        return torch.bmm(a_t.view(M, S, L).transpose(0, 1),
                         b_t.view(N, S, L).permute(1, 2, 0)).sum(0)
    w1f = w1.float()
    A, Cm = w1f[:, :H], w1f[:, 2 * H:3 * H]
    gq = buf.s1 @ (A + Cm) + buf.dq2
    Gq = buf.s1.t() @ q
    db1 = buf.s1.sum(0)
    if hand:
        # one split-K pass for G, dW2, db2, dw3, db3 (dr_din_mlp_wgrad)
        gout, wout = n1 * 2 * H, n2 * n1
        out = torch.empty(gout + wout + 2 * n2 + 1, dtype=torch.float32, device=dev)
        wsb = lib().dr_din_mlp_wgrad_workspace_size(n1, 2 * H, n2)
        ws = workspace(wsb, dev)
        check(lib().dr_din_mlp_wgrad_valid(ptr(buf.da1t), ptr(buf.xt), ptr(buf.da2t),
                                           ptr(buf.h1t), ptr(buf.h2t), ptr(buf.dsc), cap,
                                           ptr(buf.off[B:]), n1, 2 * H, n2, ptr(out), ptr(ws), wsb,
                                           stream_handle(dev)))
        _post(dev)
        G = out[:gout].view(n1, 2 * H)
        dW2 = out[gout:gout + wout].view(n2, n1)
        db2 = out[gout + wout:gout + wout + n2]
        dw3 = out[gout + wout + n2:gout + wout + 2 * n2].view(1, n2)
        db3 = out[gout + wout + 2 * n2:].view(1)
    else:
        G = kred(buf.da1t, buf.xt)
        dW2 = kred(buf.da2t, buf.h1t)
        db2 = buf.da2t.sum(1)
        dw3 = (buf.h2t @ buf.dsc).view(1, n2)
        db3 = buf.dsc.sum().view(1)
    Gf, Gqf = G[:, :H], G[:, H:]
    dW1 = torch.cat([Gq, Gf, Gq - Gf, Gqf], 1)
    return gq, dW1, db1, dW2, db2, dw3, db3


def din_dice_forward(x, alpha, epsilon):
    """Dice (utils.py:12-35) over a [B, n] fp32 batch in one kernel
    (dr_din_dice_forward) -> (y [B, n], stats [2, n] = column mean, std)."""
    dev = _dev(x)
    B, n = x.shape
    xc, a = _c(x, torch.float32), _c(alpha, torch.float32)
    y = torch.empty((B, n), dtype=torch.float32, device=dev)
    st = torch.empty((2, n), dtype=torch.float32, device=dev)
    check(lib().dr_din_dice_forward(ptr(xc), ptr(a), B, n, float(epsilon), ptr(y), ptr(st),
                                    stream_handle(dev)))
    _post(dev)
    return y, st


def din_dice_backward(x, grad_y, alpha, stats, epsilon):
    """-> (grad_x [B, n], grad_alpha [n]) through the batch statistics."""
    dev = _dev(x)
    B, n = x.shape
    xc, g, a = _c(x, torch.float32), _c(grad_y, torch.float32), _c(alpha, torch.float32)
    gx = torch.empty((B, n), dtype=torch.float32, device=dev)
    ga = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib().dr_din_dice_backward(ptr(xc), ptr(g), ptr(a), ptr(_c(stats, torch.float32)), B, n,
                                     float(epsilon), ptr(gx), ptr(ga), stream_handle(dev)))
    _post(dev)
    return gx, ga


def din_fcn_input_forward(uid, item, his_sum, att, gamma, beta, scale):
    """Model_DIN's fcn input + inference batch_normalization in one pass
    (dr_din_fcn_input_forward) -> [B, Du + 4H]."""
    dev = _dev(item)
    B, H = item.shape
    Du = uid.shape[1]
    u, i, h, a = (_c(t, torch.float32) for t in (uid, item, his_sum, att))
    gm, bt = _c(gamma, torch.float32), _c(beta, torch.float32)
    out = torch.empty((B, Du + 4 * H), dtype=torch.float32, device=dev)
    check(lib().dr_din_fcn_input_forward(ptr(u), ptr(i), ptr(h), ptr(a), ptr(gm), ptr(bt), B, Du,
                                         H, float(scale), ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def din_fcn_input_backward(grad, uid, item, his_sum, att, gamma, scale):
    """-> (g_uid, g_item, g_his_sum, g_att, g_gamma, g_beta)."""
    dev = _dev(item)
    B, H = item.shape
    Du = uid.shape[1]
    g = _c(grad, torch.float32)
    u, i, h, a = (_c(t, torch.float32) for t in (uid, item, his_sum, att))
    gm = _c(gamma, torch.float32)
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    gu, gi, gh, ga, gg, gb = e(B, Du), e(B, H), e(B, H), e(B, H), e(Du + 4 * H), e(Du + 4 * H)
    check(lib().dr_din_fcn_input_backward(ptr(g), ptr(u), ptr(i), ptr(h), ptr(a), ptr(gm), B, Du,
                                          H, float(scale), ptr(gu), ptr(gi), ptr(gh), ptr(ga),
                                          ptr(gg), ptr(gb), stream_handle(dev)))
    _post(dev)
    return gu, gi, gh, ga, gg, gb


def din_attention_pool(scores, mask, facts, with_sum=True):
    """Masked softmax over the history + weighted sum (din_attention, mode
    'SUM', utils.py:286-303) and the history sum (model.py:98) in one pass.
    scores / mask [B, T], facts [B, T, H] -> (att [B, H], his_sum [B, H] or
    None, alphas [B, T])."""
    dev = _dev(facts)
    B, T, H = facts.shape
    s, m, f = _c(scores, torch.float32), _c(mask, torch.float32), _c(facts, torch.float32)
    att = torch.empty((B, H), dtype=torch.float32, device=dev)
    hs = torch.empty((B, H), dtype=torch.float32, device=dev) if with_sum else None
    al = torch.empty((B, T), dtype=torch.float32, device=dev)
    check(lib().dr_din_attention_pool(ptr(s), ptr(m), ptr(f), B, T, H, ptr(att), ptr(hs), ptr(al),
                                      stream_handle(dev)))
    _post(dev)
    return att, hs, al


def din_attention_pool_grad(alphas, mask, facts, grad_att, grad_sum=None, out=None):
    """-> (grad_scores [B, T], grad_facts [B, T, H]); out: a contiguous fp32
    [B, T, H] buffer to write grad_facts into (e.g. a slice of the lookup's
    gradient)."""
    dev = _dev(facts)
    B, T, H = facts.shape
    a, m, f = _c(alphas, torch.float32), _c(mask, torch.float32), _c(facts, torch.float32)
    ga = _c(grad_att, torch.float32)
    gs = None if grad_sum is None else _c(grad_sum, torch.float32)
    gsc = torch.empty((B, T), dtype=torch.float32, device=dev)
    if out is not None:
        if out.shape != (B, T, H) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous fp32 [B, T, H] tensor")
        gf = out
    else:
        gf = torch.empty((B, T, H), dtype=torch.float32, device=dev)
    check(lib().dr_din_attention_pool_grad(ptr(a), ptr(m), ptr(f), ptr(ga), ptr(gs), B, T, H,
                                           ptr(gsc), ptr(gf), stream_handle(dev)))
    _post(dev)
    return gsc, gf


# ---------------------------------------------------------------------------
# GRU / attention-gated GRU over a padded sequence (DIEN's interest layers:
# dynamic_rnn(GRUCell) and dynamic_rnn(VecAttGRUCell))
# ---------------------------------------------------------------------------
GRU_MAX_HIDDEN = 64
# DR_GRU=torch: the torch composition of the same contract on the GPU too (A/B)
_GRU_NATIVE = os.environ.get("DR_GRU", "native") != "torch"


def gru_native_ok(xp):
    """The kernels take this input: fp32 on a GPU, H a multiple of 4 in [4, 64]."""
    H = xp.shape[2] // 3
    return (xp.is_cuda and xp.dtype == torch.float32 and xp.shape[0] >= 1 and xp.shape[1] >= 1
            and H % 4 == 0 and 4 <= H <= GRU_MAX_HIDDEN)


def gru_seq_forward(xp, wh_g, wh_c, seq_len, att=None):
    """dr_gru_seq_forward: xp [B, T, 3H] (x W_x + b; columns r | u | c), wh_g
    [H, 2H], wh_c [H, H], seq_len [B], att [B, T] or None -> (out [B, T, H],
    h_final [B, H], saved [B, T, 3H] = r | u | c per valid step, zeros after)."""
    dev = _dev(xp)
    B, T, H3 = xp.shape
    H = H3 // 3
    x, wg, wc = _c(xp, torch.float32), _c(wh_g, torch.float32), _c(wh_c, torch.float32)
    sl = _c(seq_len, torch.int32)
    a = None if att is None else _c(att, torch.float32)
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    out, hf = e(B, T, H), e(B, H)
    saved = e(lib().dr_gru_seq_saved_size(B, T, H) // 4).view(B, T, H3)
    check(lib().dr_gru_seq_forward(ptr(x), ptr(wg), ptr(wc), ptr(sl), ptr(a), B, T, H, ptr(out),
                                   ptr(hf), ptr(saved), stream_handle(dev)))
    _post(dev)
    return out, hf, saved


def gru_seq_backward(wh_g, wh_c, seq_len, att, out, saved, grad_out, grad_h_final,
                     need_grad_att=True):
    """dr_gru_seq_backward -> (grad_xp [B, T, 3H], grad_att [B, T] or None);
    grad_out / grad_h_final may be None (zeros)."""
    dev = _dev(out)
    B, T, H = out.shape
    wg, wc = _c(wh_g, torch.float32), _c(wh_c, torch.float32)
    sl = _c(seq_len, torch.int32)
    a = None if att is None else _c(att, torch.float32)
    go = None if grad_out is None else _c(grad_out, torch.float32)
    gh = None if grad_h_final is None else _c(grad_h_final, torch.float32)
    gxp = torch.empty((B, T, 3 * H), dtype=torch.float32, device=dev)
    ga = (torch.empty((B, T), dtype=torch.float32, device=dev)
          if a is not None and need_grad_att else None)
    check(lib().dr_gru_seq_backward(ptr(wg), ptr(wc), ptr(sl), ptr(a), ptr(_c(out, torch.float32)),
                                    ptr(_c(saved, torch.float32)), ptr(go), ptr(gh), B, T, H,
                                    ptr(gxp), ptr(ga), stream_handle(dev)))
    _post(dev)
    return gxp, ga


class _GruSequenceFn(torch.autograd.Function):
    """One launch each way (dr_gru_seq_forward / _backward); the state-weight
    gradients are two GEMMs over what the kernels leave."""

    @staticmethod
    def forward(ctx, xp, wh_g, wh_c, seq_len, att):
        out, hf, saved = gru_seq_forward(xp, wh_g, wh_c, seq_len, att)
        ctx.save_for_backward(wh_g, wh_c, seq_len, att, out, saved)
        return out, hf

    @staticmethod
    def backward(ctx, g_out, g_hf):
        wh_g, wh_c, seq_len, att, out, saved = ctx.saved_tensors
        B, T, H = out.shape
        need_att = att is not None and ctx.needs_input_grad[4]
        gxp, ga = gru_seq_backward(wh_g, wh_c, seq_len, att, out, saved, g_out, g_hf, need_att)
        dwg = dwc = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            hp = torch.zeros_like(out)
            hp[:, 1:] = out[:, :-1]
            hp = hp.view(B * T, H)
            g2 = gxp.view(B * T, 3 * H)
            dwg = hp.t() @ g2[:, :2 * H]
            dwc = (saved.view(B * T, 3 * H)[:, :H] * hp).t() @ g2[:, 2 * H:]
        return gxp, dwg, dwc, None, ga


def _gru_sequence_torch(xp, wh_g, wh_c, seq_len, att=None):
    """The contract of dr_gru_seq_forward as a torch composition (autograd
    forms the backward): CPU tensors, widths outside the kernels' set, and
    the DR_GRU=torch arm."""
    B, T, H3 = xp.shape
    H = H3 // 3
    h = xp.new_zeros(B, H)
    lens = seq_len.to(xp.device).reshape(B, 1)
    outs = []
    for t in range(T):
        x = xp[:, t]
        g = torch.sigmoid(x[:, :2 * H] + h @ wh_g)
        r, u = g[:, :H], g[:, H:]
        c = torch.tanh(x[:, 2 * H:] + (r * h) @ wh_c)
        if att is not None:
            u = (1.0 - att[:, t:t + 1]) * u
        nh = u * h + (1.0 - u) * c
        live = t < lens
        outs.append(torch.where(live, nh, torch.zeros_like(nh)))
        h = torch.where(live, nh, h)
    return torch.stack(outs, 1), h


def gru_sequence(xp, wh_g, wh_c, seq_len, att=None):
    """GRU (att None) or attention-gated GRU (AUGRU) over a padded sequence
    with dynamic_rnn(sequence_length=seq_len) semantics -> (out [B, T, H],
    h_final [B, H]); gradients for xp, wh_g, wh_c and att.  xp [B, T, 3H] is
    x W_x + b with columns r | u | c; TF's cell: c = tanh(xp_c + (r h) wh_c).
    fp32 GPU tensors with H a multiple of 4 up to 64 run one HIP kernel each
    way; anything else (and DR_GRU=torch) the torch composition."""
    if xp.dim() != 3 or xp.shape[2] % 3:
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT, "gru_sequence: xp must be [B, T, 3H]")
    if _GRU_NATIVE and gru_native_ok(xp):
        return _GruSequenceFn.apply(xp, wh_g, wh_c, seq_len, att)
    return _gru_sequence_torch(xp, wh_g, wh_c, seq_len, att)


# ---------------------------------------------------------------------------
# Multi-head self-attention over a padded history (BST's attention block: the
# reference multihead_attention, key masking then query masking; DESIGN
# section 26)
# ---------------------------------------------------------------------------
MHA_HEAD_DIMS = (8, 16, 32)
MHA_MAX_T = 128
# DR_MHA=torch: the torch composition of the same contract on the GPU too (A/B)
_MHA_NATIVE = os.environ.get("DR_MHA", "native") != "torch"


def mha_native_ok(q, heads):
    """The kernels take this input: fp32 [B >= 1, 1 <= T <= 128, heads *
    head_dim] on a GPU with head_dim 8, 16 or 32."""
    if q.dim() != 3 or heads < 1 or q.shape[2] % heads:
        return False
    return (q.is_cuda and q.dtype == torch.float32 and q.shape[0] >= 1
            and 1 <= q.shape[1] <= MHA_MAX_T and q.shape[2] // heads in MHA_HEAD_DIMS)


def _mha_qkv(q, k, v):
    """q, k, v as the kernels read them: (q, k, v, ld) unchanged when they are
    fp32 row views with one row stride (the column blocks of a packed
    projection), contiguous copies otherwise."""
    B, T, E = q.shape
    ld = q.stride(1)
    for t in (q, k, v):
        if not (t.dtype == torch.float32 and t.shape == q.shape and t.stride(2) == 1
                and t.stride(1) == ld and t.stride(0) == T * ld and ld % 4 == 0 and ld >= E
                and t.data_ptr() % 16 == 0):
            return _c(q, torch.float32), _c(k, torch.float32), _c(v, torch.float32), E
    return q, k, v, ld


def mha_seq_forward(q, k, v, seq_len, heads, scale=None):
    """dr_mha_seq_forward: q, k, v [B, T, heads * head_dim] (row views with a
    common stride pass without a copy), seq_len [B] -> (out [B, T, E], saved
    [B, heads, T] = the rows' logsumexp); zeros at t >= seq_len[b]."""
    dev = _dev(q)
    B, T, E = q.shape
    hd = E // heads
    scale = float(hd) ** -0.5 if scale is None else float(scale)
    q, k, v, ld = _mha_qkv(q, k, v)
    sl = _c(seq_len, torch.int32)
    out = torch.empty((B, T, E), dtype=torch.float32, device=dev)
    saved = torch.empty((B, heads, T), dtype=torch.float32, device=dev)
    check(lib().dr_mha_seq_forward(ptr(q), ptr(k), ptr(v), ld, ptr(sl), B, T, heads, hd, scale,
                                   ptr(out), ptr(saved), stream_handle(dev)))
    _post(dev)
    return out, saved


def mha_seq_backward(q, k, v, seq_len, heads, out, saved, grad_out, scale=None):
    """dr_mha_seq_backward -> (grad_q, grad_k, grad_v), the three column blocks
    of one packed [B, T, 3E] buffer; zeros at t >= seq_len[b]."""
    dev = _dev(q)
    B, T, E = q.shape
    hd = E // heads
    scale = float(hd) ** -0.5 if scale is None else float(scale)
    q, k, v, ld = _mha_qkv(q, k, v)
    sl = _c(seq_len, torch.int32)
    g = torch.empty((B, T, 3 * E), dtype=torch.float32, device=dev)
    gq, gk, gv = g[..., :E], g[..., E:2 * E], g[..., 2 * E:]
    check(lib().dr_mha_seq_backward(ptr(q), ptr(k), ptr(v), ld, ptr(sl),
                                    ptr(_c(out, torch.float32)), ptr(_c(saved, torch.float32)),
                                    ptr(_c(grad_out, torch.float32)), B, T, heads, hd, scale,
                                    ptr(gq), ptr(gk), ptr(gv), 3 * E, stream_handle(dev)))
    _post(dev)
    return gq, gk, gv


class _MultiheadAttentionFn(torch.autograd.Function):
    """One launch each way (dr_mha_seq_forward / _backward)."""

    @staticmethod
    def forward(ctx, q, k, v, seq_len, heads):
        out, saved = mha_seq_forward(q, k, v, seq_len, heads)
        ctx.save_for_backward(q, k, v, seq_len, out, saved)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, g_out):
        q, k, v, seq_len, out, saved = ctx.saved_tensors
        gq, gk, gv = mha_seq_backward(q, k, v, seq_len, ctx.heads, out, saved, g_out)
        return gq, gk, gv, None, None


def _multihead_attention_torch(q, k, v, seq_len, heads):
    """The contract of dr_mha_seq_forward as a torch composition (autograd
    forms the backward), in the reference's order: scale, key masking with
    -2**32 + 1, softmax, query masking, weighted sum.  CPU tensors, shapes
    outside the kernels' set, and the DR_MHA=torch arm."""
    B, T, E = q.shape
    hd = E // heads
    split = lambda x: x.reshape(B, T, heads, hd).permute(0, 2, 1, 3)  # noqa: E731
    lens = seq_len.to(q.device).clamp(0, T)
    live = torch.arange(T, device=q.device)[None, :] < lens[:, None]                # [B, T]
    s = (split(q) @ split(k).transpose(2, 3)) * (float(hd) ** -0.5)                # [B, h, T, T]
    s = torch.where(live[:, None, None, :], s, torch.full_like(s, float(-2 ** 32 + 1)))
    p = torch.softmax(s, -1) * live[:, None, :, None].to(s.dtype)
    return (p @ split(v)).permute(0, 2, 1, 3).reshape(B, T, E)


def multihead_attention(q, k, v, seq_len, heads):
    """Multi-head self-attention over a padded history -> out [B, T, E]:
    softmax(q k^T / sqrt(head_dim)) v per head over the first seq_len[b] keys,
    exact zeros at the padded queries; gradients for q, k and v (views of one
    packed buffer on the native path).  q, k, v [B, T, E = heads * head_dim]
    may be the column blocks of one packed projection.  fp32 GPU tensors with
    head_dim 8 / 16 / 32 and T <= 128 run one HIP kernel each way; anything
    else (and DR_MHA=torch) the torch composition."""
    if q.dim() != 3 or heads < 1 or q.shape[2] % heads or k.shape != q.shape or v.shape != q.shape:
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT,
                                "multihead_attention: q, k, v must be [B, T, heads * head_dim]")
    if _MHA_NATIVE and mha_native_ok(q, heads):
        return _MultiheadAttentionFn.apply(q, k, v, seq_len, heads)
    return _multihead_attention_torch(q, k, v, seq_len, heads)


# ---------------------------------------------------------------------------
# Gate softmax and expert mixing (the block of the multi-task models MMoE and
# PLE: per task a softmax gate over the experts it may see, and the gate-
# weighted mixture of the expert outputs)
# ---------------------------------------------------------------------------
GATE_MIX_MAX = (8, 16, 512)             # tasks, experts, expert width
# DR_GATE_MIX=torch: the torch composition of the same contract on the GPU too (A/B)
_GATE_MIX_NATIVE = os.environ.get("DR_GATE_MIX", "native") != "torch"


def gate_mix_native_ok(logits, experts):
    """The kernels take this input: fp32 [B >= 1, K <= 8, E <= 16] and [B, E,
    H] on a GPU with H a multiple of 4 in [4, 512]."""
    if logits.dim() != 3 or experts.dim() != 3:
        return False
    (B, K, E), H = logits.shape, experts.shape[2]
    return (logits.is_cuda and logits.dtype == torch.float32 and experts.dtype == torch.float32
            and B >= 1 and 1 <= K <= GATE_MIX_MAX[0] and 1 <= E <= GATE_MIX_MAX[1]
            and H % 4 == 0 and 4 <= H <= GATE_MIX_MAX[2])


def _gate_mix_rows(x):
    """[B, N, W] as the kernels read it, rows of N * W floats: (x, row stride)
    unchanged for an fp32 view with one row stride (a column block of a wider
    buffer), a copy with the row stride rounded up to 4 floats otherwise (K * E
    need not be a multiple of 4)."""
    B, N, W = x.shape
    ld = -(-N * W // 4) * 4
    if (x.dtype == torch.float32 and x.stride(2) == 1 and (N == 1 or x.stride(1) == W)
            and (x.stride(0) >= ld and x.stride(0) % 4 == 0 if B > 1 else ld == N * W)
            and x.data_ptr() % 16 == 0):
        return x, (x.stride(0) if B > 1 else ld)
    rows = torch.empty((B, ld), dtype=torch.float32, device=x.device)
    rows[:, :N * W] = x.reshape(B, N * W)
    return rows, ld


def _gate_mix_select(select, K, E):
    """select (None, or a [K, E] bool tensor or nested list) as the K host
    words of the C entries (bit e of word k: task k sees expert e) and as the
    bool tensor."""
    if select is None or isinstance(select, C.Array):      # (already the words)
        return select, None
    sel = torch.as_tensor(select, dtype=torch.bool).cpu()
    if sel.shape != (K, E):
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT, "gate_mix: select must be [tasks, experts]")
    words = (sel.long() << torch.arange(E)).sum(1).tolist()
    return (C.c_uint32 * K)(*words), sel


def gate_mix_forward(logits, experts, select=None):
    """dr_gate_mix_forward: logits [B, K, E], experts [B, E, H] (views with a
    row stride pass without a copy) -> (out [B, K, H], gates [B, K, E])."""
    dev = _dev(experts)
    (B, K, E), H = logits.shape, experts.shape[2]
    z, ld_z = _gate_mix_rows(logits)
    h, ld_h = _gate_mix_rows(experts)
    words, _ = _gate_mix_select(select, K, E)
    out = torch.empty((B, K, H), dtype=torch.float32, device=dev)
    gates = torch.empty(lib().dr_gate_mix_saved_size(B, K, E) // 4, dtype=torch.float32,
                        device=dev).view(B, K, E)
    check(lib().dr_gate_mix_forward(ptr(z), ld_z, ptr(h), ld_h, words, B, K, E, H, ptr(out),
                                    ptr(gates), stream_handle(dev)))
    _post(dev)
    return out, gates


def gate_mix_backward(experts, gates, grad_out, select=None):
    """dr_gate_mix_backward -> (grad_logits [B, K, E], grad_experts [B, E, H])."""
    dev = _dev(experts)
    (B, K, E), H = gates.shape, experts.shape[2]
    h, ld_h = _gate_mix_rows(experts)
    go, ld_go = _gate_mix_rows(grad_out)
    words, _ = _gate_mix_select(select, K, E)
    gz = torch.empty((B, K, E), dtype=torch.float32, device=dev)
    gh = torch.empty((B, E, H), dtype=torch.float32, device=dev)
    check(lib().dr_gate_mix_backward(ptr(h), ld_h, ptr(_c(gates, torch.float32)), ptr(go), ld_go,
                                     words, B, K, E, H, ptr(gz), ptr(gh), stream_handle(dev)))
    _post(dev)
    return gz, gh


class _GateMixFn(torch.autograd.Function):
    """One launch each way (dr_gate_mix_forward / _backward); the gates are
    the only saved extra."""

    @staticmethod
    def forward(ctx, logits, experts, select):
        ctx.select = _gate_mix_select(select, logits.shape[1], logits.shape[2])[0]
        out, gates = gate_mix_forward(logits, experts, ctx.select)
        ctx.save_for_backward(experts, gates)
        ctx.mark_non_differentiable(gates)
        return out, gates

    @staticmethod
    def backward(ctx, g_out, _g_gates):
        experts, gates = ctx.saved_tensors
        gz, gh = gate_mix_backward(experts, gates, g_out, ctx.select)
        return gz, gh, None


def _gate_mix_torch(logits, experts, select=None):
    """The contract of dr_gate_mix_forward as a torch composition (autograd
    forms the backward) -> (out, gates): CPU tensors, shapes outside the
    kernels' set, and the DR_GATE_MIX=torch arm."""
    _, sel = _gate_mix_select(select, logits.shape[1], logits.shape[2])
    z = logits
    if sel is not None:
        z = z.masked_fill(~sel.to(z.device), float("-inf"))
    gates = torch.softmax(z, -1)
    return torch.bmm(gates, experts), gates


def gate_mix(logits, experts, select=None):
    """The multi-gate mixture of experts -> out [B, K, H]: out[b, k] = sum_e
    softmax_e(logits[b, k])[e] * experts[b, e], the softmax over the experts
    task k may see (select [K, E] bool tensor or nested list; None = all) and
    exactly 0 on the others; gradients for logits and experts.  Both inputs
    may be views with a row stride (the output of one Linear, a column block).
    fp32 GPU tensors with K <= 8, E <= 16 and H a multiple of 4 up to 512 run
    one HIP kernel each way; anything else (and DR_GATE_MIX=torch) the torch
    composition."""
    if (logits.dim() != 3 or experts.dim() != 3 or logits.shape[0] != experts.shape[0]
            or logits.shape[2] != experts.shape[1]):
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT,
                                "gate_mix: logits must be [B, K, E] and experts [B, E, H]")
    if _GATE_MIX_NATIVE and gate_mix_native_ok(logits, experts):
        return _GateMixFn.apply(logits, experts, select)[0]
    return _gate_mix_torch(logits, experts, select)[0]


# ---------------------------------------------------------------------------
# Layer normalisation with a residual add in front and a relu and P
# elementwise masks behind (BST's normalize, every MaskBlock of MaskNet;
# DESIGN section 28)
# ---------------------------------------------------------------------------
LAYER_NORM_MAX = (1024, 8)              # width, masks
# DR_LAYER_NORM=torch: the torch composition of the same contract on the GPU too (A/B)
_LAYER_NORM_NATIVE = os.environ.get("DR_LAYER_NORM", "native") != "torch"


def layer_norm_native_ok(x, gain, bias, residual=None, mask=None):
    """The kernels take this input: fp32 GPU tensors, x [B >= 1, D] with D a
    multiple of 4 in [4, 1024], and at most 8 masks [B, P, D]."""
    ts = [t for t in (x, gain, bias, residual, mask) if t is not None]
    if x.dim() != 2 or not all(t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    B, D = x.shape
    return (B >= 1 and D % 4 == 0 and 4 <= D <= LAYER_NORM_MAX[0]
            and (mask is None or 1 <= mask.shape[1] <= LAYER_NORM_MAX[1]))


def _layer_norm_rows(x):
    """[B, D] or [B, P, D] as the kernels read it, (x, row stride) or (NULL,
    0) for None: _gate_mix_rows' rule, a column block passes without a copy."""
    if x is None:
        return None, 0
    return _gate_mix_rows(x if x.dim() == 3 else x.unsqueeze(1))


def layer_norm_forward(x, gain, bias, eps, residual=None, mask=None, relu=False):
    """dr_layer_norm_forward -> (out [B, D] or [B, P, D], saved [B, 2] = (mean,
    rstd)); x, residual and mask may be views with a row stride."""
    dev = _dev(x)
    B, D = x.shape
    P = 1 if mask is None else mask.shape[1]
    xs, ld_x = _layer_norm_rows(x)
    rs, ld_r = _layer_norm_rows(residual)
    ms, ld_m = _layer_norm_rows(mask)
    out = torch.empty((B, D) if mask is None else (B, P, D), dtype=torch.float32, device=dev)
    saved = torch.empty(lib().dr_layer_norm_saved_size(B) // 4, dtype=torch.float32,
                        device=dev).view(B, 2)
    check(lib().dr_layer_norm_forward(ptr(xs), ld_x, ptr(rs), ld_r, ptr(_c(gain, torch.float32)),
                                      ptr(_c(bias, torch.float32)), ptr(ms), ld_m, B, D, P,
                                      float(eps), int(bool(relu)), ptr(out), ptr(saved),
                                      stream_handle(dev)))
    _post(dev)
    return out, saved


def layer_norm_backward(x, gain, bias, saved, grad_out, residual=None, mask=None, relu=False):
    """dr_layer_norm_backward -> (grad_x [B, D], grad_mask [B, P, D] or None,
    grad_gain [D], grad_bias [D]); the gradient of residual is grad_x."""
    dev = _dev(x)
    B, D = x.shape
    P = 1 if mask is None else mask.shape[1]
    xs, ld_x = _layer_norm_rows(x)
    rs, ld_r = _layer_norm_rows(residual)
    ms, ld_m = _layer_norm_rows(mask)
    go, ld_go = _layer_norm_rows(grad_out)
    gx = torch.empty((B, D), dtype=torch.float32, device=dev)
    gm = None if mask is None else torch.empty((B, P, D), dtype=torch.float32, device=dev)
    gg = torch.empty(D, dtype=torch.float32, device=dev)
    gb = torch.empty(D, dtype=torch.float32, device=dev)
    nbytes = lib().dr_layer_norm_workspace_size(B, D)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    check(lib().dr_layer_norm_backward(ptr(xs), ld_x, ptr(rs), ld_r, ptr(_c(gain, torch.float32)),
                                       ptr(_c(bias, torch.float32)), ptr(ms), ld_m,
                                       ptr(_c(saved, torch.float32)), ptr(go), ld_go, B, D, P,
                                       int(bool(relu)), ptr(gx), ptr(gm), ptr(gg), ptr(gb),
                                       ptr(ws), nbytes, stream_handle(dev)))
    _post(dev)
    return gx, gm, gg, gb


class _LayerNormFn(torch.autograd.Function):
    """One launch forward, one plus the finishing launch backward; (mean,
    rstd) per row is the only saved extra."""

    @staticmethod
    def forward(ctx, x, gain, bias, residual, mask, eps, relu):
        out, saved = layer_norm_forward(x, gain, bias, eps, residual, mask, relu)
        ctx.save_for_backward(x, gain, bias, saved, residual, mask)
        ctx.relu = relu
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, gain, bias, saved, residual, mask = ctx.saved_tensors
        gx, gm, gg, gb = layer_norm_backward(x, gain, bias, saved, g_out, residual, mask, ctx.relu)
        return gx, gg, gb, (None if residual is None else gx), gm, None, None


def _layer_norm_torch(x, gain, bias, eps, residual=None, mask=None, relu=False):
    """The contract of dr_layer_norm_forward as a torch composition (autograd
    forms the backward): CPU tensors, shapes and dtypes outside the kernels'
    set, and the DR_LAYER_NORM=torch arm."""
    s = x if residual is None else x + residual
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    a = gain * (s - mean) / (var + eps) ** 0.5 + bias
    if relu:
        a = torch.relu(a)
    return a if mask is None else a.unsqueeze(1) * mask


def layer_norm(x, gain, bias, eps, residual=None, mask=None, relu=False):
    """Layer normalisation of s = x + residual over the last axis (biased
    variance, eps inside the root), gain and bias, an optional relu, and an
    optional product with P masks: x, residual [B, D], gain, bias [D] -> [B, D],
    or [B, P, D] = a[:, None] * mask with mask [B, P, D] (x is read once for
    all P outputs).  Gradients for x, residual, gain, bias and mask.  x,
    residual and mask may be column blocks of wider buffers.  fp32 GPU tensors
    with D a multiple of 4 in [4, 1024] and P <= 8 run the HIP kernels;
    anything else (and DR_LAYER_NORM=torch) the torch composition."""
    if (x.dim() != 2 or gain.shape != x.shape[1:] or bias.shape != x.shape[1:]
            or (residual is not None and residual.shape != x.shape)
            or (mask is not None and (mask.dim() != 3 or mask.shape[0] != x.shape[0]
                                      or mask.shape[2] != x.shape[1]))):
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT,
                                "layer_norm: x and residual must be [B, D], gain and bias [D] "
                                "and mask [B, P, D]")
    if _LAYER_NORM_NATIVE and layer_norm_native_ok(x, gain, bias, residual, mask):
        return _LayerNormFn.apply(x, gain, bias, residual, mask, eps, relu)
    return _layer_norm_torch(x, gain, bias, eps, residual, mask, relu)


# ---------------------------------------------------------------------------
# One layer of xDeepFM's Compressed Interaction Network
# ---------------------------------------------------------------------------
CIN_MAX = (64, 64, 256)                 # width D, fields m, maps (in and out)
CIN_TORCH_Z_BYTES = 256 << 20           # the composition's outer product per chunk of B
# DR_CIN=torch: the torch composition of the same contract on the GPU too (A/B)
_CIN_NATIVE = os.environ.get("DR_CIN", "native") != "torch"


def cin_native_ok(x0, xk, weight):
    """The kernels take this input: fp32 GPU tensors, x0 [B >= 1, m, D], xk [B,
    Hk, D], weight [Hn, Hk, m] with D, m <= 64 and Hk, Hn <= 256."""
    if not all(t.is_cuda and t.dtype == torch.float32 for t in (x0, xk, weight)):
        return False
    (B, m, D), Hk, Hn = x0.shape, xk.shape[1], weight.shape[0]
    return (B >= 1 and 1 <= D <= CIN_MAX[0] and 1 <= m <= CIN_MAX[1]
            and 1 <= Hk <= CIN_MAX[2] and 1 <= Hn <= CIN_MAX[2])


def cin_forward(x0, xk, weight, bias=None):
    """dr_cin_forward -> out [B, Hn, D]; xk may be x0 itself (the first layer)."""
    dev = _dev(x0)
    (B, m, D), Hk, Hn = x0.shape, xk.shape[1], weight.shape[0]
    x0c = _c(x0, torch.float32)
    xkc = x0c if xk is x0 else _c(xk, torch.float32)
    out = torch.empty((B, Hn, D), dtype=torch.float32, device=dev)
    check(lib().dr_cin_forward(ptr(x0c), ptr(xkc), ptr(_c(weight, torch.float32)),
                               ptr(None if bias is None else _c(bias, torch.float32)), B, m, Hk,
                               Hn, D, ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def cin_backward(x0, xk, weight, grad_out, with_bias=True):
    """dr_cin_backward -> (grad_xk [B, Hk, D], grad_x0 [B, m, D], grad_weight
    [Hn, Hk, m], grad_bias [Hn] or None); when xk is x0 the caller adds the
    first two."""
    dev = _dev(x0)
    (B, m, D), Hk, Hn = x0.shape, xk.shape[1], weight.shape[0]
    x0c = _c(x0, torch.float32)
    xkc = x0c if xk is x0 else _c(xk, torch.float32)
    gxk = torch.empty((B, Hk, D), dtype=torch.float32, device=dev)
    gx0 = torch.empty((B, m, D), dtype=torch.float32, device=dev)
    gw = torch.empty((Hn, Hk, m), dtype=torch.float32, device=dev)
    gb = torch.empty(Hn, dtype=torch.float32, device=dev) if with_bias else None
    nbytes = lib().dr_cin_workspace_size(B, m, Hk, Hn, D)
    ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=dev)
    check(lib().dr_cin_backward(ptr(x0c), ptr(xkc), ptr(_c(weight, torch.float32)),
                                ptr(_c(grad_out, torch.float32)), B, m, Hk, Hn, D, ptr(gxk),
                                ptr(gx0), ptr(gw), ptr(gb), ptr(ws), nbytes, stream_handle(dev)))
    _post(dev)
    return gxk, gx0, gw, gb


class _CinLayerFn(torch.autograd.Function):
    """One launch forward; backward one launch for the input gradients, one and
    a finishing launch for the weight and bias gradients.  Nothing is saved
    but the inputs."""

    @staticmethod
    def forward(ctx, x0, xk, weight, bias):
        ctx.save_for_backward(x0, weight) if xk is None else ctx.save_for_backward(x0, weight, xk)
        ctx.with_bias = bias is not None
        return cin_forward(x0, x0 if xk is None else xk, weight, bias)

    @staticmethod
    def backward(ctx, g_out):
        x0, weight = ctx.saved_tensors[:2]
        first = len(ctx.saved_tensors) == 2
        xk = x0 if first else ctx.saved_tensors[2]
        gxk, gx0, gw, gb = cin_backward(x0, xk, weight, g_out, ctx.with_bias)
        return (gx0 + gxk, None, gw, gb) if first else (gx0, gxk, gw, gb)


def _cin_layer_torch(x0, xk, weight, bias=None):
    """The contract of dr_cin_forward as a torch composition (autograd forms
    the backward): CPU tensors, other dtypes, shapes outside the kernels' set
    and the DR_CIN=torch arm.  Z[b, (i, j), d] = xk[b, i, d] x0[b, j, d] is
    formed by broadcasting and multiplied by W.view(Hn, Hk m), over chunks of
    B that keep Z under CIN_TORCH_Z_BYTES."""
    (B, m, D), Hk, Hn = x0.shape, xk.shape[1], weight.shape[0]
    w = weight.reshape(Hn, Hk * m)
    step = max(1, CIN_TORCH_Z_BYTES // max(1, Hk * m * D * x0.element_size()))
    outs = []
    for lo in range(0, max(B, 1), step):
        z = (xk[lo:lo + step, :, None, :] * x0[lo:lo + step, None, :, :]).reshape(-1, Hk * m, D)
        outs.append(torch.matmul(w, z))
    out = outs[0] if len(outs) == 1 else torch.cat(outs, 0)
    return out if bias is None else out + bias[:, None]


def cin_layer(x0, xk, weight, bias=None):
    """One Compressed Interaction Network layer (xDeepFM): out[b, h, d] =
    bias[h] + sum_{i, j} weight[h, i, j] xk[b, i, d] x0[b, j, d] with x0 [B, m,
    D], xk [B, Hk, D] (x0 itself in the first layer), weight [Hn, Hk, m], bias
    [Hn] or None -> [B, Hn, D]; gradients for all of them.  fp32 contiguous
    GPU tensors with D, m <= 64 and Hk, Hn <= 256 run the HIP kernels, which
    never store the outer product; anything else (and DR_CIN=torch) the torch
    composition."""
    if (x0.dim() != 3 or xk.dim() != 3 or weight.dim() != 3 or xk.shape[0] != x0.shape[0]
            or xk.shape[2] != x0.shape[2] or weight.shape[1] != xk.shape[1]
            or weight.shape[2] != x0.shape[1]
            or (bias is not None and bias.shape != weight.shape[:1])):
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT,
                                "cin_layer: x0 must be [B, m, D], xk [B, Hk, D], weight [Hn, Hk, "
                                "m] and bias [Hn]")
    if (_CIN_NATIVE and cin_native_ok(x0, xk, weight)
            and (bias is None or (bias.is_cuda and bias.dtype == torch.float32))):
        return _CinLayerFn.apply(x0, None if xk is x0 else xk, weight, bias)
    return _cin_layer_torch(x0, xk, weight, bias)


# ---------------------------------------------------------------------------
# CAN's co-action unit: a per-sample micro-MLP over a history
# ---------------------------------------------------------------------------
CO_ACTION_MAX = (3, 32, 4)              # layers, width, orders
# DR_CO_ACTION=torch: the torch composition of the same contract on the GPU too (A/B)
_CO_ACTION_NATIVE = os.environ.get("DR_CO_ACTION", "native") != "torch"


def co_action_param_len(widths, orders, bias=False, order_indep=False):
    """P: the floats of one sample's weights."""
    per = sum(a * b + (b if bias else 0) for a, b in zip(widths[:-1], widths[1:]))
    return per * (orders if order_indep else 1)


def co_action_native_ok(param, his, mask, widths, orders):
    """The kernels take this input: fp32 GPU tensors, B >= 1, T >= 1, 1 to 3
    layers of widths that are multiples of 4 in [4, 32], orders in [1, 4]."""
    if not all(t.is_cuda and t.dtype == torch.float32 for t in (param, his, mask)):
        return False
    L, D, O = CO_ACTION_MAX
    return (his.shape[0] >= 1 and his.shape[1] >= 1 and 2 <= len(widths) <= L + 1
            and all(4 <= d <= D and d % 4 == 0 for d in widths) and 1 <= orders <= O
            and his.numel() < 2 ** 31)


def _co_action_rows(param, his):
    """param and his as the kernels read them: (param, ld_param, his, ld_his),
    unchanged when they are fp32 views with a contiguous last dimension, one
    row stride that is a multiple of 4 and a 16-byte aligned start (the column
    blocks of a merged lookup), contiguous copies otherwise."""
    B, T, d0 = his.shape
    if not (param.dtype == torch.float32 and param.stride(1) == 1 and param.stride(0) % 4 == 0
            and param.stride(0) >= param.shape[1] and param.data_ptr() % 16 == 0):
        param = _c(param, torch.float32)
    if not (his.dtype == torch.float32 and his.stride(2) == 1 and his.stride(1) % 4 == 0
            and his.stride(1) >= d0 and his.stride(0) == T * his.stride(1)
            and his.data_ptr() % 16 == 0):
        his = _c(his, torch.float32)
    return param, param.stride(0), his, his.stride(1)


def _co_action_widths(widths):
    return (C.c_int * len(widths))(*[int(d) for d in widths])


def co_action_forward(param, his, mask, widths, orders, bias=False, order_indep=False):
    """dr_co_action_forward -> out [B, orders * sum(widths[1:])]."""
    dev = _dev(his)
    B, T, _ = his.shape
    param, ld_p, his, ld_h = _co_action_rows(param, his)
    out = torch.empty((B, orders * sum(widths[1:])), dtype=torch.float32, device=dev)
    check(lib().dr_co_action_forward(ptr(param), ld_p, ptr(his), ld_h, ptr(_c(mask, torch.float32)),
                                     B, T, _co_action_widths(widths), len(widths) - 1, orders,
                                     int(bias), int(order_indep), ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def co_action_backward(param, his, mask, grad_out, widths, orders, bias=False, order_indep=False):
    """dr_co_action_backward -> (grad_his [B, T, d0], grad_param [B, P]), both
    dense and written in full."""
    dev = _dev(his)
    B, T, d0 = his.shape
    param, ld_p, his, ld_h = _co_action_rows(param, his)
    gh = torch.empty((B, T, d0), dtype=torch.float32, device=dev)
    gp = torch.empty((B, param.shape[1]), dtype=torch.float32, device=dev)
    check(lib().dr_co_action_backward(ptr(param), ld_p, ptr(his), ld_h,
                                      ptr(_c(mask, torch.float32)),
                                      ptr(_c(grad_out, torch.float32)), B, T,
                                      _co_action_widths(widths), len(widths) - 1, orders, int(bias),
                                      int(order_indep), ptr(gh), ptr(gp), stream_handle(dev)))
    _post(dev)
    return gh, gp


class _CoActionFn(torch.autograd.Function):
    """One launch each way; nothing is saved but the inputs (the backward
    recomputes the activations tile by tile)."""

    @staticmethod
    def forward(ctx, param, his, mask, widths, orders, bias, order_indep):
        ctx.save_for_backward(param, his, mask)
        ctx.cfg = (widths, orders, bias, order_indep)
        return co_action_forward(param, his, mask, *ctx.cfg)

    @staticmethod
    def backward(ctx, g_out):
        param, his, mask = ctx.saved_tensors
        gh, gp = co_action_backward(param, his, mask, g_out, *ctx.cfg)
        return gp, gh, None, None, None, None, None


def _co_action_torch(param, his, mask, widths, orders, bias=False, order_indep=False):
    """The contract of dr_co_action_forward as a torch composition (autograd
    forms the backward): CPU tensors, other dtypes, widths outside the kernels'
    set and the DR_CO_ACTION=torch arm.  A position with mask 0 is replaced by
    zeros before it is used, as the kernels skip it."""
    B = his.shape[0]
    live = (mask != 0).unsqueeze(-1)
    his = torch.where(live, his, torch.zeros_like(his))
    m = mask.to(his.dtype).unsqueeze(-1)
    outs, at = [], 0
    for p in range(1, orders + 1):
        if not order_indep:
            at = 0
        h = his ** p
        for j, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
            h = torch.bmm(h, param[:, at:at + a * b].reshape(B, a, b))
            at += a * b
            if bias:
                h = h + param[:, None, at:at + b]
                at += b
            if j + 2 < len(widths):
                h = torch.tanh(h)
            outs.append((h * m).sum(1))
    return torch.cat(outs, 1)


def co_action(param, his, mask, widths=(16, 8, 4), orders=3, bias=False, order_indep=False):
    """CAN's co-action unit (the reference's gen_coaction, mode "can"): param
    [B, P] holds, per sample, the weights of a small MLP of widths (d0, ...,
    dL) -- per set, for every layer W_j [d(j-1), d(j)] row-major, then b_j if
    bias; one set, or one per order with order_indep.  For p = 1..orders the
    MLP (tanh between the layers, none after the last) runs on his ** p, his
    [B, T, d0], and every layer's activations are summed over the positions
    with mask [B, T] -> [B, orders * sum(widths[1:])]; a position with mask 0
    is not read.  Gradients for param and his.  param and his may be column
    blocks of wider buffers.  fp32 GPU tensors with at most 3 layers, widths
    that are multiples of 4 up to 32 and orders <= 4 run one HIP kernel each
    way; anything else (and DR_CO_ACTION=torch) the torch composition."""
    widths = tuple(int(d) for d in widths)
    if (his.dim() != 3 or param.dim() != 2 or mask.dim() != 2 or len(widths) < 2 or orders < 1
            or min(widths) < 1 or his.shape[2] != widths[0] or mask.shape != his.shape[:2]
            or param.shape != (his.shape[0],
                               co_action_param_len(widths, orders, bias, order_indep))):
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT,
                                "co_action: his must be [B, T, widths[0]], mask [B, T] and param "
                                "[B, P] with P the weights of the widths, orders and sets")
    if _CO_ACTION_NATIVE and co_action_native_ok(param, his, mask, widths, orders):
        return _CoActionFn.apply(param, his, mask, widths, int(orders), bool(bias),
                                 bool(order_indep))
    return _co_action_torch(param, his, mask, widths, int(orders), bias, order_indep)


# ---------------------------------------------------------------------------
# FiBiNET's bilinear interaction over every pair of fields
# ---------------------------------------------------------------------------
BILINEAR_MAX = (64, 64)                 # fields m, width D
BILINEAR_KINDS = ("all", "each", "interaction")
# DR_BILINEAR=torch: the torch composition of the same contract on the GPU too (A/B)
_BILINEAR_NATIVE = os.environ.get("DR_BILINEAR", "native") != "torch"


def bilinear_native_ok(x, weight, scale=None):
    """The kernels take this input: fp32 GPU tensors, x [B >= 1, m, D] with
    2 <= m <= 64 and 1 <= D <= 64, weight [*, D, D], scale [B, m] or None."""
    ts = (x, weight) if scale is None else (x, weight, scale)
    if not all(t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    B, m, D = x.shape
    return B >= 1 and 2 <= m <= BILINEAR_MAX[0] and 1 <= D <= BILINEAR_MAX[1]


def bilinear_forward(x, weight, kind, scale=None):
    """dr_bilinear_forward -> out [B, m (m - 1) / 2, D]."""
    dev = _dev(x)
    B, m, D = x.shape
    out = torch.empty((B, m * (m - 1) // 2, D), dtype=torch.float32, device=dev)
    check(lib().dr_bilinear_forward(ptr(_c(x, torch.float32)),
                                    ptr(None if scale is None else _c(scale, torch.float32)),
                                    ptr(_c(weight, torch.float32)), BILINEAR_KINDS.index(kind), B,
                                    m, D, ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def bilinear_backward(x, weight, kind, grad_out, scale=None):
    """dr_bilinear_backward -> (grad_x [B, m, D], grad_scale [B, m] or None,
    grad_weight of weight's shape)."""
    dev = _dev(x)
    B, m, D = x.shape
    k = BILINEAR_KINDS.index(kind)
    gx = torch.empty((B, m, D), dtype=torch.float32, device=dev)
    gs = None if scale is None else torch.empty((B, m), dtype=torch.float32, device=dev)
    gw = torch.empty(tuple(weight.shape), dtype=torch.float32, device=dev)
    nbytes = lib().dr_bilinear_workspace_size(k, B, m, D)
    ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=dev)
    check(lib().dr_bilinear_backward(ptr(_c(x, torch.float32)),
                                     ptr(None if scale is None else _c(scale, torch.float32)),
                                     ptr(_c(weight, torch.float32)),
                                     ptr(_c(grad_out, torch.float32)), k, B, m, D, ptr(gx),
                                     ptr(gs), ptr(gw), ptr(ws), nbytes, stream_handle(dev)))
    _post(dev)
    return gx, gs, gw


class _BilinearFn(torch.autograd.Function):
    """One launch forward; backward one launch for grad_x and grad_scale, one
    and a finishing launch for grad_weight.  Nothing is saved but the inputs."""

    @staticmethod
    def forward(ctx, x, weight, scale, kind):
        ctx.save_for_backward(x, weight) if scale is None else ctx.save_for_backward(x, weight,
                                                                                     scale)
        ctx.kind = kind
        return bilinear_forward(x, weight, kind, scale)

    @staticmethod
    def backward(ctx, g_out):
        x, weight = ctx.saved_tensors[:2]
        scale = ctx.saved_tensors[2] if len(ctx.saved_tensors) == 3 else None
        gx, gs, gw = bilinear_backward(x, weight, ctx.kind, g_out, scale)
        return gx, gw, gs, None


def _bilinear_torch(x, weight, kind, scale=None):
    """The contract of dr_bilinear_forward as a torch composition (autograd
    forms the backward): CPU tensors, other dtypes, shapes outside the
    kernels' set and the DR_BILINEAR=torch arm."""
    m = x.shape[1]
    idx = torch.triu_indices(m, m, 1, device=x.device)
    v = x if scale is None else x * scale.unsqueeze(-1)
    if kind == "interaction":
        u = torch.matmul(v[:, idx[0]].unsqueeze(2), weight).squeeze(2)
    else:
        # weight [1 or m, D, D] broadcasts over the fields
        u = torch.matmul(v.unsqueeze(2), weight).squeeze(2)[:, idx[0]]
    return u * v[:, idx[1]]


def bilinear_interaction(x, weight, kind="interaction", scale=None):
    """FiBiNET's bilinear interaction: x [B, m, D] field embeddings, v = x or
    scale[:, :, None] * x with scale [B, m] (SENET's weights), and for every
    pair i < j in itertools.combinations' order out[b, p, :] = (v_i W) * v_j
    -> [B, m (m - 1) / 2, D], with W = weight[0] (kind "all", weight [1, D,
    D]), weight[i] ("each", [m, D, D]) or weight[p] ("interaction", [P, D,
    D]).  Gradients for x, weight and scale.  fp32 contiguous GPU tensors with
    2 <= m <= 64 and D <= 64 run the HIP kernels, which write the output once
    and store nothing else; anything else (and DR_BILINEAR=torch) the torch
    composition."""
    ok = kind in BILINEAR_KINDS and x.dim() == 3 and weight.dim() == 3 and x.shape[1] >= 2
    if ok:
        B, m, D = x.shape
        n = {"all": 1, "each": m, "interaction": m * (m - 1) // 2}[kind]
        ok = tuple(weight.shape) == (n, D, D) and (scale is None or tuple(scale.shape) == (B, m))
    if not ok:
        raise _lib.DeepRecError(_lib.INVALID_ARGUMENT,
                                "bilinear_interaction: x must be [B, m >= 2, D], scale [B, m] and "
                                "weight [1, D, D] (kind all), [m, D, D] (each) or [m (m - 1) / 2, "
                                "D, D] (interaction)")
    if _BILINEAR_NATIVE and bilinear_native_ok(x, weight, scale):
        return _BilinearFn.apply(x, weight, scale, kind)
    return _bilinear_torch(x, weight, kind, scale)


# ---------------------------------------------------------------------------
# Row-sharded exchange helpers
# ---------------------------------------------------------------------------
def partition_by_owner(keys, world, n_dev=None):
    """Stable bucket of keys by owner = key % world (SOK selectKernel,
    all2all_input_dispatcher.cu:36-126; EV rule embedding_ops.py:207-209).
    Returns (keys_sorted, perm, send_counts[world] int64)."""
    dev = _dev(keys)
    k = _c(keys, torch.int64)
    n = k.numel()
    ko = torch.empty_like(k)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(world, dtype=torch.int64, device=dev)
    wsb = lib().dr_partition_workspace_size(n)
    ws = workspace(wsb, dev)
    check(lib().dr_partition_by_owner(ptr(k), n, ptr(n_dev), world, ptr(ko), ptr(perm),
                                      ptr(counts), ptr(ws), wsb, stream_handle(dev)))
    _post(dev)
    return ko, perm, counts


def partition_by_owner_mod(keys, world, premod, n_dev=None):
    """partition_by_owner with owner = (key % premod) % world (floor mods):
    premod = 1000 is the EV partition rule ids % 1000 % np
    (python/ops/embedding_ops.py:207-209)."""
    dev = _dev(keys)
    k = _c(keys, torch.int64)
    n = k.numel()
    ko = torch.empty_like(k)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(world, dtype=torch.int64, device=dev)
    wsb = lib().dr_partition_workspace_size(n)
    ws = workspace(wsb, dev)
    check(lib().dr_partition_by_owner_mod(ptr(k), n, ptr(n_dev), world, int(premod), ptr(ko),
                                          ptr(perm), ptr(counts), ptr(ws), wsb,
                                          stream_handle(dev)))
    _post(dev)
    return ko, perm, counts


def rows_scatter(src, perm, out, n_dev=None):
    """out[perm[j]] = src[j]"""
    dev = _dev(src)
    check(lib().dr_rows_scatter(ptr(src), ptr(perm), perm.numel(), ptr(n_dev), src.shape[1],
                                ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def rows_pack(src, perm, out, n_dev=None):
    """out[j] = src[perm[j]]"""
    dev = _dev(src)
    check(lib().dr_rows_pack(ptr(src), ptr(perm), perm.numel(), ptr(n_dev), src.shape[1],
                             ptr(out), stream_handle(dev)))
    _post(dev)
    return out


def fill_synthetic(table, seed):
    """table[r, c] = hash(seed, r, c) in [-1, 1) (regenerable: synth_value)."""
    dev = _dev(table)
    check(lib().dr_fill_synthetic(ptr(table), table.shape[0], table.shape[1], seed,
                                  stream_handle(dev)))
    return table


def synth_value(seed, row, col):
    return lib().dr_synth_value(seed, row, col)
