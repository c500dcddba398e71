"""A numpy model of the dense checkpoint entries (csrc/dense_ckpt.hip): the
update marks of a dense table (one bit per row in ceil(rows / 32) uint32
words), mark / mark all / clear / count / export / upsert, and the tensors a
full save and a delta of a dense table and its slots hold.  Pinned on
hand-worked cases by tests/test_dense_ckpt_ref.py; the GPU tests compare the C
entries and the Python surface with it bit for bit."""
import numpy as np

INCR = "sparse_incr_"


def words(rows):
    return 0 if rows <= 0 else (rows + 31) // 32


def tail_mask(rows):
    r = rows % 32
    return (1 << r) - 1 if r else 0xFFFFFFFF


def valid_mask(w, rows):
    nw = words(rows)
    if w < 0 or w >= nw:
        return 0
    return tail_mask(rows) if w == nw - 1 else 0xFFFFFFFF


def new_bits(rows):
    return np.zeros(words(rows), np.uint32)


def effective(n, n_dev):
    return n if n_dev is None else max(min(n, int(n_dev)), 0)


def mark(bits, rows, idx, n_dev=None):
    """bits with every in-range idx[i], i < min(len(idx), n_dev), set.  What
    lies at or past the count is never looked at."""
    bits = bits.copy()
    r = np.asarray(idx, dtype=np.int64).reshape(-1)[:effective(len(idx), n_dev)]
    r = r[(r >= 0) & (r < rows)]
    np.bitwise_or.at(bits, r >> 5, (np.uint32(1) << (r & 31).astype(np.uint32)))
    return bits


def mark_all(rows):
    return np.array([valid_mask(w, rows) for w in range(words(rows))], np.uint32)


def marked_rows(bits, rows):
    """The marked rows in ascending order; bits at or past `rows` are ignored."""
    nw = words(rows)
    v = np.asarray(bits[:nw], dtype=np.uint32).copy()
    if nw:
        v[nw - 1] &= np.uint32(tail_mask(rows))
    flags = np.unpackbits(v.astype("<u4").view(np.uint8), bitorder="little")
    return np.flatnonzero(flags).astype(np.int64)


def count(bits, rows):
    return int(marked_rows(bits, rows).size)


def export(bits, rows, cols, capacity):
    """(m, rows_out [min(m, capacity)], [cols[c][rows_out] ...])."""
    r = marked_rows(bits, rows)
    k = r[:capacity]
    return int(r.size), k, [np.asarray(c)[k] for c in cols]


def upsert(cols, rows, idx, vals, n_dev=None):
    """(new cols, latched): cols[c][idx[i]] = vals[c][i] for i < N, an index
    outside [0, rows) skipped and latched."""
    cols = [np.array(c, copy=True) for c in cols]
    latched = False
    for i in range(effective(len(idx), n_dev)):
        r = int(idx[i])
        if 0 <= r < rows:
            for c, v in zip(cols, vals):
                c[r] = v[i]
        else:
            latched = True
    return cols, latched


def full_tensors(key, weight, slots=()):
    """{tensor name: array} of a full save: the table under `key` and each
    (name, array) slot under key/name, whole."""
    out = {key: np.asarray(weight)}
    for name, a in slots:
        out["%s/%s" % (key, name)] = np.asarray(a)
    return out


def delta_tensors(key, bits, weight, slots=()):
    """{tensor name: array} of a delta: for the table and each slot,
    NAME-sparse_incr_keys (the marked rows ascending) and
    NAME-sparse_incr_values (their rows; a [rows] slot gives [m])."""
    rows = np.asarray(weight).shape[0]
    r = marked_rows(bits, rows)
    out = {}
    for name, a in [(key, weight)] + [("%s/%s" % (key, n), a) for n, a in slots]:
        out["%s-%skeys" % (name, INCR)] = r
        out["%s-%svalues" % (name, INCR)] = np.asarray(a)[r]
    return out
