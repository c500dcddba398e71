"""Reference of the MultiHashVariable ("Q-R") lookups and their gradient:
numpy int64 / fp32 for the index rule, the combine and the gradient split,
composed with the CPU oracle's pieces (unique, gather, the segment reductions
and their gradients, the dense applies) exactly as the reference's graph
composes them.  `orc` is the oracle module (tests/conftest.py fixture)."""
import numpy as np

OPS = ("add", "mul", "concat")


def index(ids, q_rows, r_rows):
    """q = floordiv(id, Q rows), r = floormod(id, R rows) on int64 (numpy's
    // and % floor, as Python's); ok = q is a row of the Q table."""
    ids = np.asarray(ids, np.int64)
    q = ids // np.int64(q_rows)
    r = ids % np.int64(r_rows)
    return q, r, (q >= 0) & (q < q_rows)


def dim_of(Qt, Rt, op):
    return Qt.shape[1] + Rt.shape[1] if op == "concat" else Qt.shape[1]


def rows(orc, Qt, Rt, op, ids):
    """Combined rows [n, dim] of ids: one fp32 operation per element; an id
    whose q is out of range is a zero row."""
    Qt = np.ascontiguousarray(Qt, np.float32)
    Rt = np.ascontiguousarray(Rt, np.float32)
    ids = np.asarray(ids, np.int64).reshape(-1)
    q, r, ok = index(ids, Qt.shape[0], Rt.shape[0])
    a = orc.gather(Qt, np.where(ok, q, 0)) if ids.size else np.zeros((0, Qt.shape[1]), np.float32)
    b = orc.gather(Rt, r) if ids.size else np.zeros((0, Rt.shape[1]), np.float32)
    if op == "add":
        out = a + b
    elif op == "mul":
        out = a * b
    elif op == "concat":
        out = np.concatenate([a, b], 1)
    else:
        raise ValueError(op)
    out = out.astype(np.float32)
    out[~ok] = 0.0
    return out


def materialize(orc, Qt, Rt, op, n_ids):
    """The dense table the variable stands for: row id = combined row of id."""
    return rows(orc, Qt, Rt, op, np.arange(n_ids, dtype=np.int64))


def lookup(orc, Qt, Rt, op, ids):
    ids = np.asarray(ids, np.int64)
    return rows(orc, Qt, Rt, op, ids).reshape(ids.shape + (dim_of(Qt, Rt, op),))


def _unique_rows(orc, Qt, Rt, op, values):
    values = np.ascontiguousarray(values, np.int64)
    if values.size == 0:
        return values, np.zeros(0, np.int32), np.zeros((0, dim_of(Qt, Rt, op)), np.float32)
    uids, idx = orc.unique(values)
    return uids, idx, rows(orc, Qt, Rt, op, uids)


def lookup_sparse(orc, Qt, Rt, op, indices, values, batch, weights=None, combiner="mean"):
    """embedding_lookup_sparse: unique -> combined rows of the unique ids ->
    the oracle's pooled reduce over them (SparseSegment* in the ALI order, or
    the weighted composition)."""
    uids, idx, emb = _unique_rows(orc, Qt, Rt, op, values)
    if uids.size == 0:
        out = np.zeros((batch, dim_of(Qt, Rt, op)), np.float32)
        if weights is not None and combiner != "sum":
            out[:] = np.nan
        return out
    return orc.embedding_lookup_sparse(emb, indices, idx.astype(np.int64), batch, weights=weights,
                                       combiner=combiner)


def split(Qt, Rt, op, uids, gu):
    """(q_idx, q_val, r_idx, r_val): the two IndexedSlices the per-unique-id
    gradient gu [U, dim] becomes.  Out-of-range q: index -1, zero rows."""
    Qt = np.ascontiguousarray(Qt, np.float32)
    Rt = np.ascontiguousarray(Rt, np.float32)
    gu = np.ascontiguousarray(gu, np.float32)
    q, r, ok = index(uids, Qt.shape[0], Rt.shape[0])
    qc, rc = np.where(ok, q, 0), np.where(ok, r, 0)
    if op == "add":
        qv, rv = gu.copy(), gu.copy()
    elif op == "mul":
        qv = (gu * Rt[rc]).astype(np.float32)
        rv = (gu * Qt[qc]).astype(np.float32)
    elif op == "concat":
        qv, rv = gu[:, :Qt.shape[1]].copy(), gu[:, Qt.shape[1]:].copy()
    else:
        raise ValueError(op)
    qv[~ok] = 0.0
    rv[~ok] = 0.0
    return np.where(ok, q, -1), qv, np.where(ok, r, -1), rv


def lookup_sparse_grad(orc, Qt, Rt, op, indices, values, batch, top_grad, weights=None,
                       combiner="mean"):
    """Backward of lookup_sparse: (uids, gu, q_idx, q_val, r_idx, r_val); gu is
    the per-unique-id gradient in UnsortedSegmentSum order (the oracle's
    embedding_lookup_sparse_grad over the combined rows)."""
    uids, idx, emb = _unique_rows(orc, Qt, Rt, op, values)
    pos, gu = orc.embedding_lookup_sparse_grad(emb, indices, idx.astype(np.int64), batch, top_grad,
                                               weights=weights, combiner=combiner)
    assert np.array_equal(pos, np.arange(uids.size))
    return (uids, gu) + split(Qt, Rt, op, uids, gu)


def dedup(orc, idx, val):
    """_deduplicate_indexed_slices (optimizer.py:68-83): unique + segment sum;
    index -1 (skipped slices) dropped first."""
    idx = np.asarray(idx, np.int64)
    keep = idx >= 0
    idx, val = idx[keep], np.ascontiguousarray(val, np.float32)[keep]
    if idx.size == 0:
        return idx, val
    u, pos = orc.unique(idx)
    return u, orc.unsorted_segment_sum(val, pos, u.size)


def apply_sgd(orc, table, lr, idx, val):
    u, g = dedup(orc, idx, val)
    if u.size:
        orc.dense_apply_sgd(table, np.float32(lr), g, u)


def apply_adagrad(orc, table, accum, lr, idx, val):
    u, g = dedup(orc, idx, val)
    if u.size:
        orc.dense_apply_adagrad(table, accum, np.float32(lr), g, u)
