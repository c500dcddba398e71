"""Reference of the AdaptiveEmbeddingVariable lookups and their gradient: a
numpy model of the contract.  The per-id rule (the first
position of an id decides its mask and its bucket row), the rows served by a
dict-backed EV (with the Counter filter's rule) over a hash-bucket table, the
pooling through the CPU oracle's segment reductions as multihash_ref.py does,
and the split of the per-unique-id gradient.  `orc` is the oracle module
(tests/conftest.py fixture)."""
import numpy as np


def bucket(ids, bucket_size):
    """floormod(id, bucket_size) on int64 (numpy's % floors, as Python's)."""
    return np.asarray(ids, np.int64) % np.int64(bucket_size)


class DictEV(object):
    """EmbeddingVar::LookupOrCreate / Lookup over dicts.  filter_freq > 0 is the
    Counter filter (embedding_filter.h:296-320): a key is known from its first
    sight; while freq < filter_freq a lookup adds its count to freq and serves
    the default; once freq >= filter_freq (checked BEFORE the add) the lookup
    serves the key's row, creating it from the default offered at that
    lookup."""

    def __init__(self, dim, filter_freq=0):
        self.dim = dim
        self.filter_freq = int(filter_freq)
        self.rows = {}
        self.freq = {}
        self.order = []          # keys in row-allocation order

    def lookup_or_create(self, keys, defaults, counts=None):
        """-> (out [n, dim], from_ev bool [n])."""
        keys = np.asarray(keys, np.int64)
        out = np.empty((keys.size, self.dim), np.float32)
        from_ev = np.zeros(keys.size, bool)
        for i, k in enumerate(keys.tolist()):
            c = 1 if counts is None else int(counts[i])
            if self.filter_freq:
                f = self.freq.setdefault(k, 0)
                if f < self.filter_freq:
                    self.freq[k] = f + c
                    out[i] = defaults[i]
                    continue
            if k not in self.rows:
                self.rows[k] = np.array(defaults[i], np.float32)
                self.order.append(k)
            out[i] = self.rows[k]
            from_ev[i] = True
        return out, from_ev

    def find(self, keys, defaults):
        """Read-only: the stored row of an admitted key that has one, else the
        default; nothing changes."""
        keys = np.asarray(keys, np.int64)
        out = np.empty((keys.size, self.dim), np.float32)
        from_ev = np.zeros(keys.size, bool)
        for i, k in enumerate(keys.tolist()):
            ok = k in self.rows and self.freq.get(k, 0) >= self.filter_freq
            out[i] = self.rows[k] if ok else defaults[i]
            from_ev[i] = ok
        return out, from_ev

    def export(self):
        """(keys ascending, rows, freqs)."""
        keys = np.array(sorted(self.rows), np.int64)
        rows = np.stack([self.rows[k] for k in keys.tolist()]) if keys.size else \
            np.zeros((0, self.dim), np.float32)
        freqs = np.array([self.freq.get(k, 0) for k in keys.tolist()], np.int64)
        return keys, rows.astype(np.float32), freqs


def per_id(orc, values, mask, bucket_size, hash_rows=None):
    """The per-id rule.  -> (uids [U] first-occurrence order, idx [nnz], counts
    [U], m_u bool [U], h_u int64 [U], bad: a supplied bucket row was out of
    range and replaced by row 0)."""
    values = np.ascontiguousarray(values, np.int64)
    mask = np.asarray(mask).reshape(-1)
    assert mask.size == values.size
    if values.size == 0:
        z = np.zeros(0, np.int64)
        return z, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, bool), z, False
    uids, idx, counts = orc.unique(values, with_counts=True)
    first = np.full(uids.size, values.size, np.int64)
    np.minimum.at(first, idx.astype(np.int64), np.arange(values.size, dtype=np.int64))
    m_u = mask[first] != 0
    if hash_rows is None:
        h_u = bucket(uids, bucket_size)
    else:
        h_u = np.asarray(hash_rows, np.int64).reshape(-1)[first]
    ok = (h_u >= 0) & (h_u < bucket_size)
    return uids, idx, counts, m_u, np.where(ok, h_u, 0), bool((~ok).any())


def served(orc, H, ev, values, mask, hash_rows=None, read_only=False):
    """Rows served for the unique ids: a dict with uids, idx, m_u, h_u, emb
    [U, dim], ev_keys / ev_src (the stable compaction of the EV ids), bad."""
    H = np.ascontiguousarray(H, np.float32)
    uids, idx, counts, m_u, h_u, bad = per_id(orc, values, mask, H.shape[0], hash_rows)
    emb = H[h_u].astype(np.float32) if uids.size else np.zeros((0, H.shape[1]), np.float32)
    ev_src = np.flatnonzero(m_u).astype(np.int32)
    ev_keys = uids[ev_src]
    if ev_src.size:
        defaults = emb[ev_src].copy()          # the hash rows as the table stands now
        if read_only:
            rows, _ = ev.find(ev_keys, defaults)
        else:
            rows, _ = ev.lookup_or_create(ev_keys, defaults,
                                          counts[ev_src] if ev.filter_freq else None)
        emb[ev_src] = rows
    return dict(uids=uids, idx=idx, m_u=m_u, h_u=h_u, emb=emb, ev_keys=ev_keys, ev_src=ev_src,
                bad=bad)


def pool(orc, emb, idx, indices, batch, weights=None, combiner="mean"):
    """The oracle's pooled reduce over the served rows (SparseSegment* in the
    ALI order, or the weighted composition)."""
    if emb.shape[0] == 0:
        out = np.zeros((batch, emb.shape[1]), np.float32)
        if weights is not None and combiner != "sum":
            out[:] = np.nan
        return out
    return orc.embedding_lookup_sparse(np.ascontiguousarray(emb, np.float32), indices,
                                       idx.astype(np.int64), batch, weights=weights,
                                       combiner=combiner)


def lookup_sparse(orc, H, ev, indices, values, batch, mask, hash_rows=None, weights=None,
                  combiner="mean", read_only=False):
    s = served(orc, H, ev, values, mask, hash_rows, read_only)
    return pool(orc, s["emb"], s["idx"], indices, batch, weights, combiner), s


def split(gu, m_u, h_u, uids):
    """The two IndexedSlices of the per-unique-id gradient gu [U, dim]:
    (ev_keys [Ue], ev_vals [Ue, dim]) compacted in ascending u, and
    (hash_idx [U] = h_u or -1, hash_vals = gu itself)."""
    gu = np.ascontiguousarray(gu, np.float32)
    src = np.flatnonzero(m_u)
    return (np.asarray(uids, np.int64)[src], gu[src].copy(),
            np.where(m_u, -1, h_u).astype(np.int64), gu)


def lookup_sparse_grad(orc, s, indices, batch, top_grad, weights=None, combiner="mean"):
    """Backward of lookup_sparse over the forward's record s: (gu, ev_keys,
    ev_vals, hash_idx, hash_vals); gu is the per-unique-id gradient in
    UnsortedSegmentSum order."""
    pos, gu = orc.embedding_lookup_sparse_grad(np.ascontiguousarray(s["emb"], np.float32), indices,
                                               s["idx"].astype(np.int64), batch, top_grad,
                                               weights=weights, combiner=combiner)
    assert np.array_equal(pos, np.arange(s["uids"].size))
    return (gu,) + split(gu, s["m_u"], s["h_u"], s["uids"])
