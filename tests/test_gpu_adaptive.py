"""AdaptiveEmbeddingVariable on the GPU: the pooled and
unpooled lookups, the gradient slices and the training step against

  * the twin -- a second EmbeddingVariable plus a DenseTable, driven only
    through ops that existed before: unique on the host, ev2.sparse_read(ev ids,
    ev_init_value = the hash rows), a stitched [U, D] DenseTable and
    embedding_lookup_sparse over idx; hand-built IndexedSlices in the backward;
  * tests/adaptive_ref.py, the numpy model of the contract.

Every comparison is bit equality (NaNs must coincide).

Shapes are the smallest at which each piece can go wrong: B = 64, bucket_size
5, ids in [0, 49) plus -7 and 2^40 + 3 (the floor mod of a negative and of a
64-bit id); row widths 4, 6, 16, 128, 260 (vector / scalar layouts, one and
several chunks per lane); bag lengths 0, 1, 2, 7, 8, 9, 10, 16, 17, 33 with a
repeat inside every longer bag; masks all 0, all 1, by id parity, random per
id, and random per id with one repeated id whose later position disagrees
with its first.

The Counter filter compares freq BEFORE adding the lookup's count (the EV's
own rule): with filter_freq = 3 an id that occurs twice per lookup is served
its hash row on sights 1-2 (freq 0 -> 2 -> 4) and its EV row from sight 3; an
id that occurs once per lookup reaches freq 3 at sight 3 and has its row from
sight 4.  Both are checked."""
import numpy as np
import pytest
import torch

import adaptive_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, BUCKET, NIDS = 64, 5, 49
ODD_IDS = (-7, (1 << 40) + 3)
LENS = [0, 1, 2, 7, 8, 9, 10, 16, 17, 33]
DIMS = (4, 6, 16, 128, 260)
COMBINERS = ("sum", "mean", "sqrtn")
MASKS = ("zeros", "ones", "parity", "random", "disagree")
_N = [0]


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    from deeprec_amd import get_adaptive_embedding_variable  # noqa: F401  (the feature under test)
    deeprec_amd.load()
    deeprec_amd.set_validate(True)
    assert torch.cuda.is_available()
    return deeprec_amd


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), device=DEV, dtype=dtype)


def same(a, b):
    """Bit equality of two arrays, NaNs at the same places."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def table(seed, D):
    return np.random.default_rng(seed).standard_normal((BUCKET, D)).astype(np.float32)


_CASES = {}


def bags(seed, weighted=False):
    """indices [nnz, 2], ids [nnz], weights, lens: 64 bags whose lengths go
    through LENS (then random ones), ids in [0, 49) and the two odd ids, with a
    repeat inside every longer bag."""
    key = (seed, weighted)
    if key not in _CASES:
        rng = np.random.default_rng(seed)
        lens = np.array(LENS + list(rng.choice(LENS, B - len(LENS))))
        rng.shuffle(lens)
        rows = np.repeat(np.arange(B), lens)
        cols = np.concatenate([np.arange(n) for n in lens])
        ind = np.stack([rows, cols], 1).astype(np.int64)
        ids = rng.integers(0, NIDS, rows.size).astype(np.int64)
        for j, k in enumerate(rng.choice(rows.size, 6, replace=False)):
            ids[k] = ODD_IDS[j % 2]
        for b in np.flatnonzero(lens >= 2):             # a repeat inside every longer bag
            k0 = int(np.searchsorted(rows, b))
            ids[k0 + 1] = ids[k0]
        w = rng.uniform(0.25, 2.0, rows.size).astype(np.float32) if weighted else None
        _CASES[key] = (ind, ids, w, lens)
    return _CASES[key]


def mask_of(kind, ids, seed=0):
    """A per-position mask [nnz]; every kind but "disagree" is a function of
    the id."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "zeros":
        return np.zeros(ids.size, np.int64)
    if kind == "ones":
        return np.ones(ids.size, np.int64)
    if kind == "parity":
        return (ids & 1).astype(np.int64)
    u, inv = np.unique(ids, return_inverse=True)
    m = rng.integers(0, 2, u.size)[inv].astype(np.int64)
    if kind == "disagree":
        # later positions of three repeated ids contradict their first: the first decides
        done = 0
        for x in u:
            pos = np.flatnonzero(ids == x)
            if pos.size >= 2 and done < 3:
                m[pos[1:]] = 1 - m[pos[0]]
                done += 1
        assert done == 3
    return m


def sp_of(dr, ind, vals, batch=B):
    return dr.SparseTensor(T(ind), T(vals), (batch, int(ind[:, 1].max()) + 1))


def spw_of(dr, ind, w, batch=B):
    return None if w is None else sp_of(dr, ind, w, batch)


def counter3(dr):
    return dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(filter_freq=3))


def make(dr, D, H, ev_option=None):
    _N[0] += 1
    return dr.get_adaptive_embedding_variable("ad%d" % _N[0], D, BUCKET, initializer=T(H),
                                              ev_option=ev_option, device=DEV)


class Twin(object):
    """The hand composition over a second EV and a DenseTable (ops that existed
    before this feature)."""

    def __init__(self, dr, orc, D, H, ev_option=None):
        _N[0] += 1
        self.dr, self.orc = dr, orc
        self.ev = dr.EmbeddingVariable("ad_twin%d" % _N[0], D, 0.0, ev_option=ev_option)
        self.hash = dr.DenseTable(T(H))
        self.last = None

    def lookup(self, ind, ids, mask, hash_rows=None, weights=None, combiner="mean", batch=B):
        dr = self.dr
        uids, idx, counts, m_u, h_u, _ = ref.per_id(self.orc, ids, mask, BUCKET, hash_rows)
        emb = self.hash.weight[T(h_u)].clone()                          # gather
        if m_u.any():
            cnt = T(counts[m_u]) if self.ev.filter_freq else None
            rows = self.ev.sparse_read(T(uids[m_u]), counts=cnt, ev_init_value=emb[T(m_u)])
            emb[T(m_u)] = rows                                          # stitch
        block = dr.DenseTable(emb)
        out = dr.embedding_lookup_sparse(block, sp_of(dr, ind, idx.astype(np.int64), batch),
                                         spw_of(dr, ind, weights, batch), combiner=combiner)
        self.last = (block, uids, m_u, h_u)
        return out

    def queue(self):
        """After out.backward(): the two hand-built IndexedSlices."""
        dr = self.dr
        block, uids, m_u, h_u = self.last
        (sl,) = block.pending_grads
        U = uids.size
        assert int(sl.num_valid.item()) == U
        assert np.array_equal(sl.indices[:U].cpu().numpy(), np.arange(U))
        gu = sl.values[:U]
        if m_u.any():
            self.ev.pending_grads.append(
                dr.IndexedSlices(gu[T(m_u)].contiguous(), T(uids[m_u]), unique=True))
        self.hash.pending_grads.append(dr.IndexedSlices(gu, T(np.where(m_u, -1, h_u))))
        return gu


def export_np(ev):
    return [x.cpu().numpy() for x in ev.export()]


def assert_same_ev(ev, twin_ev):
    for a, b in zip(export_np(ev), export_np(twin_ev)):
        assert same(a, b)


def model_lookup(orc, H, model, ind, ids, mask, hash_rows=None, weights=None, combiner="mean",
                 read_only=False):
    return ref.lookup_sparse(orc, H, model, ind, ids, B, mask, hash_rows, weights, combiner,
                             read_only)


# ---------------------------------------------------------------------------
# 1. pooled forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("D", DIMS)
def test_pooled_forward(dr, orc, D, combiner):
    H = table(D, D)
    v, twin, model = make(dr, D, H), Twin(dr, orc, D, H), ref.DictEV(D)
    masked = set()
    n = 0
    for kind in MASKS:
        for weighted in (False, True):
            ind, ids, w, lens = bags(5 + n % 3, weighted)
            n += 1
            assert 0 in lens and set(ODD_IDS) <= set(ids.tolist())
            mask = mask_of(kind, ids, n)
            with torch.no_grad():
                got = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), spw_of(dr, ind, w),
                                                 combiner=combiner,
                                                 adaptive_mask_tensor=T(mask))
                tw = twin.lookup(ind, ids, mask, weights=w, combiner=combiner)
            want, s = model_lookup(orc, H, model, ind, ids, mask, weights=w, combiner=combiner)
            assert got.shape == (B, D)
            assert same(got, tw), (D, combiner, kind, weighted)
            assert same(got, want), (D, combiner, kind, weighted)
            masked |= set(s["ev_keys"].tolist())
            if kind == "disagree":
                pos = {x: np.flatnonzero(ids == x) for x in s["uids"].tolist()}
                assert sum(1 for x, p in pos.items() if len(set(mask[p].tolist())) == 2) == 3
            if kind == "zeros":
                assert not s["ev_keys"].size
    dr.status_check()
    assert_same_ev(v.ev, twin.ev)
    keys, rows, _ = model.export()
    got_keys, got_rows = export_np(v.ev)[:2]
    assert np.array_equal(got_keys, keys) and same(got_rows, rows)
    assert int(v.ev.total_count()[0]) == len(masked) and set(ODD_IDS) <= masked
    assert same(v.hash_table.weight, H)                  # a lookup never writes the hash table


def test_onehot_bags_and_the_reference_entry_point(dr, orc):
    D = 16
    H = table(11, D)
    v, model = make(dr, D, H), ref.DictEV(D)
    rng = np.random.default_rng(12)
    ids = rng.integers(0, NIDS, B).astype(np.int64)
    ids[:2] = ODD_IDS
    ind = np.stack([np.arange(B), np.zeros(B, np.int64)], 1).astype(np.int64)
    mask = mask_of("random", ids, 3)
    sp = dr.SparseTensor(T(ind), T(ids), (B, 1))
    for m in (T(mask), T(mask.astype(np.int32)), T(mask.astype(bool)), T(mask.astype(np.uint8))):
        with torch.no_grad():
            got = dr.adaptive_embedding_lookup_sparse(v.hash_table, v.ev, sp, None, None,
                                                      combiner="sum", bucket_size=BUCKET,
                                                      adaptive_mask_tensor=m)
            flat = dr.embedding_lookup(v, T(ids.reshape(8, 8)),
                                       adaptive_mask_tensor=m.reshape(8, 8))
        want, s = model_lookup(orc, H, model, ind, ids, mask, combiner="sum")
        assert same(got, want) and same(got, s["emb"][s["idx"]])       # a bag of one id is its row
        assert tuple(flat.shape) == (8, 8, D) and same(flat.reshape(B, D), want)
    dr.status_check()


# ---------------------------------------------------------------------------
# 2. first touch
# ---------------------------------------------------------------------------
def test_a_graduating_id_starts_from_the_hash_row_it_has_trained(dr, orc):
    D = 16
    H = table(21, D)
    v, twin = make(dr, D, H), Twin(dr, orc, D, H)
    o1, o2 = dr.GradientDescentOptimizer(0.1), dr.GradientDescentOptimizer(0.1)
    ind, ids, _, _ = bags(22)
    ids = ids.copy()
    ids[0] = 7                                    # (bag 0 may be empty: 7 sits wherever nnz 0 is)
    assert 12 in ids and 2 in ids                 # other ids of bucket 2 keep training the row
    rng = np.random.default_rng(23)
    seven = T(np.array([7], np.int64))

    def step(mask, k):
        g = rng.standard_normal((B, D)).astype(np.float32)
        out = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), combiner="mean",
                                         adaptive_mask_tensor=T(mask))
        tw = twin.lookup(ind, ids, mask, combiner="mean")
        assert same(out, tw), k
        mid = (v.ev.sparse_read(seven, read_only=True).clone(), v.hash_table.weight[2].clone())
        out.backward(T(g))
        tw.backward(T(g))
        twin.queue()
        o1.apply_gradients([v], global_step=k)
        o2.apply_gradients([twin.ev, twin.hash], global_step=k)
        assert same(v.hash_table.weight, twin.hash.weight), k
        assert_same_ev(v.ev, twin.ev)
        return mid

    # step 1: mask 0 everywhere; the SGD step moves hash row 2 (7 % 5)
    step(np.zeros(ids.size, np.int64), 1)
    moved = v.hash_table.weight[2].clone()
    assert not same(moved, H[2]) and int(v.ev.total_count()[0]) == 0
    # step 2: 7 graduates; right after the lookup its EV row is the MOVED hash row, bit for bit
    mask = (ids == 7).astype(np.int64)
    ev_row, hash_row = step(mask, 2)
    assert same(ev_row[0], moved) and same(hash_row, moved)
    assert int(v.ev.total_count()[0]) == 1
    # step 3: the two rows have gone their own ways
    ev_row2 = v.ev.sparse_read(seven, read_only=True)[0].clone()
    assert not same(ev_row2, moved) and not same(ev_row2, v.hash_table.weight[2])
    ev_row3, hash_row3 = step(mask, 3)
    assert same(ev_row3[0], ev_row2) and not same(hash_row3, ev_row2)
    # ... and a change of the hash row does not reach an id that lives in the EV
    before = v.ev.sparse_read(seven, read_only=True)[0].clone()
    v.hash_table.weight[2].add_(1.0)
    hot = dr.SparseTensor(T(np.array([[0, 0]], np.int64)), seven, (1, 1))
    with torch.no_grad():
        got = dr.embedding_lookup_sparse(v, hot, combiner="sum", adaptive_mask_tensor=T([1]))
    assert same(got[0], before)
    dr.status_check()


# ---------------------------------------------------------------------------
# 3. Counter filter
# ---------------------------------------------------------------------------
def test_counter_filter_serves_the_hash_row_until_the_id_is_admitted(dr, orc):
    D = 6
    H = table(31, D).copy()
    v = make(dr, D, H, counter3(dr))
    twin, model = Twin(dr, orc, D, H, counter3(dr)), ref.DictEV(D, filter_freq=3)
    # id 8 twice per lookup, id 9 once, id 13 (bucket 3, like 8) never masked
    ids = np.array([8, 8, 9, 13], np.int64)
    ind = np.array([[0, 0], [1, 0], [2, 0], [3, 0]], np.int64)
    mask = np.array([1, 1, 1, 0], np.int64)
    sp = dr.SparseTensor(T(ind), T(ids), (4, 1))
    has = []
    for sight in range(1, 6):
        with torch.no_grad():
            got = dr.embedding_lookup_sparse(v, sp, combiner="sum", adaptive_mask_tensor=T(mask))
            tw = twin.lookup(ind, ids, mask, combiner="sum", batch=4)
        want, s = ref.lookup_sparse(orc, H, model, ind, ids, 4, mask, combiner="sum")
        assert same(got, tw) and same(got, want), sight
        fr, _, hr = v.ev.key_meta(np.array([8, 9, 13], np.int64))
        fr2, _, hr2 = twin.ev.key_meta(np.array([8, 9, 13], np.int64))
        assert np.array_equal(fr, fr2) and np.array_equal(hr, hr2), sight
        assert fr.tolist() == [min(2 * sight, 4), min(sight, 3), 0]
        has.append(hr.tolist())
        served_hash = same(got[0], v.hash_table.weight[3])
        assert served_hash == (sight <= 3)      # sight 3 creates the row FROM the hash row
        # the hash row moves between sights, so "EV row" and "hash row" can be told apart
        for t in (v.hash_table, twin.hash):
            t.weight.add_(0.5)
        H += np.float32(0.5)
    # id 8: its own row from sight 3 (freq 0 -> 2 -> 4); id 9: from sight 4 (1, 2, 3); 13 never
    assert has == [[False, False, False], [False, False, False], [True, False, False],
                   [True, True, False], [True, True, False]]
    row8 = v.ev.sparse_read(T(np.array([8], np.int64)), read_only=True)[0]
    assert same(row8, (table(31, D)[3] + np.float32(0.5) + np.float32(0.5)))   # hash row of sight 3
    assert_same_ev(v.ev, twin.ev)
    assert same(v.hash_table.weight, twin.hash.weight)
    dr.status_check()


# ---------------------------------------------------------------------------
# 4. gradient slices
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("D", (16, 6, 260))
def test_gradient_slices(dr, orc, D, combiner):
    H = table(41, D)
    rng = np.random.default_rng(42)
    for weighted, kind in ((False, "random"), (True, "disagree"), (False, "ones"),
                           (False, "zeros")):
        v, twin, model = make(dr, D, H), Twin(dr, orc, D, H), ref.DictEV(D)
        ind, ids, w, _ = bags(43, weighted)
        mask = mask_of(kind, ids, 4)
        g = rng.standard_normal((B, D)).astype(np.float32)
        out = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), spw_of(dr, ind, w),
                                         combiner=combiner, adaptive_mask_tensor=T(mask))
        out.backward(T(g))
        tw = twin.lookup(ind, ids, mask, weights=w, combiner=combiner)
        tw.backward(T(g))
        gu_twin = twin.queue()
        _, s = model_lookup(orc, H, model, ind, ids, mask, weights=w, combiner=combiner)
        gu, ek, evv, hi, hv = ref.lookup_sparse_grad(orc, s, ind, B, g, weights=w,
                                                     combiner=combiner)
        dr.status_check()
        U, Ue = s["uids"].size, ek.size
        assert same(gu_twin, gu)
        (se,), (sh,) = v.ev.pending_grads, v.hash_table.pending_grads
        # EV slice: the compacted keys and their gradient rows, the device count Ue, unique
        assert se.unique and int(se.num_valid.item()) == Ue
        assert np.array_equal(se.indices[:Ue].cpu().numpy(), ek) and same(se.values[:Ue], evv)
        assert tuple(se.values.shape)[1] == D and se.indices.numel() >= Ue
        if twin.ev.pending_grads:
            (te,) = twin.ev.pending_grads
            assert np.array_equal(te.indices.cpu().numpy(), ek) and same(te.values, evv)
        else:
            assert Ue == 0
        # hash slice: bucket row or -1 per unique id, -1 past the count, over gU itself
        assert not sh.unique and int(sh.num_valid.item()) == U
        assert np.array_equal(sh.indices[:U].cpu().numpy(), hi) and same(sh.values[:U], hv)
        assert (sh.indices[U:] == -1).all()
        (th,) = twin.hash.pending_grads
        assert np.array_equal(th.indices.cpu().numpy(), hi) and same(th.values, hv)
        if kind in ("random", "disagree"):
            assert 0 < Ue < U and (hi == -1).sum() == Ue
            keep = hi[hi >= 0]
            assert np.unique(keep).size < keep.size          # distinct ids share buckets
        assert same(v.hash_table.weight, H)


# ---------------------------------------------------------------------------
# 5. training
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["sgd", "adagrad"])
def test_five_training_steps_equal_the_twin_tables(dr, orc, opt_name):
    D = 16
    H = table(51, D)
    v, twin = make(dr, D, H), Twin(dr, orc, D, H)

    def opt():
        return dr.GradientDescentOptimizer(0.05) if opt_name == "sgd" else \
            dr.AdagradOptimizer(0.05, initial_accumulator_value=0.1)
    o1, o2 = opt(), opt()
    rng = np.random.default_rng(52)
    sizes = []
    for step in range(5):
        ind, ids, w, _ = bags(60 + step, step % 2 == 1)
        # ids graduate: the share of ids in the EV grows from step to step
        u = np.unique(ids)
        hot = set(u[rng.random(u.size) < 0.2 * (step + 1)].tolist())
        mask = np.array([x in hot for x in ids.tolist()], np.int64)
        g = rng.standard_normal((B, D)).astype(np.float32)
        out = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), spw_of(dr, ind, w),
                                         combiner="mean", adaptive_mask_tensor=T(mask))
        tw = twin.lookup(ind, ids, mask, weights=w, combiner="mean")
        assert same(out, tw), step
        out.backward(T(g))
        tw.backward(T(g))
        twin.queue()
        o1.apply_gradients([v], global_step=step)       # the variable itself in var_list
        o2.apply_gradients([twin.ev, twin.hash], global_step=step)
        dr.status_check()
        assert not v.ev.pending_grads and not v.hash_table.pending_grads
        assert same(v.hash_table.weight, twin.hash.weight), (opt_name, step)
        assert_same_ev(v.ev, twin.ev)
        sizes.append(int(v.ev.total_count()[0]))
    assert sizes[0] > 0 and sizes[-1] > sizes[0]          # ids did graduate
    assert not same(v.hash_table.weight, H)


# ---------------------------------------------------------------------------
# 6. one call, four kinds of feature
# ---------------------------------------------------------------------------
def test_multi_call_mixes_adaptive_ev_dense_and_multihash_features(dr, orc):
    D = 16
    H = table(61, D)
    rng = np.random.default_rng(62)

    def fresh():
        ev = dr.EmbeddingVariable("ad_mix%d" % (_N[0] + 1), D, 0.25)
        _N[0] += 1
        keys = np.arange(0, NIDS, 2, dtype=np.int64)
        ev.insert(T(keys), T(np.random.default_rng(63).standard_normal(
            (keys.size, D)).astype(np.float32)))
        return ev
    dense = dr.DenseTable(T(rng.standard_normal((NIDS, D)).astype(np.float32)))
    _N[0] += 1
    mh = dr.get_multihash_variable("ad_mh%d" % _N[0], [[7, D], [5, D]], operation="add",
                                   initializer=[T(rng.standard_normal((7, D)).astype(np.float32)),
                                                T(rng.standard_normal((5, D)).astype(np.float32))],
                                   device=DEV)
    cases = [bags(s) for s in (71, 72, 73, 74, 75)]
    nonneg = [(c[0], np.where((c[1] < 0) | (c[1] >= NIDS), 3, c[1])) for c in cases]
    masks = [mask_of("random", cases[0][1], 5), None, None, None, mask_of("parity", cases[4][1])]
    va, vb, ev = make(dr, D, H), make(dr, D, H), fresh()
    sps = [sp_of(dr, cases[0][0], cases[0][1]), sp_of(dr, *nonneg[1]), sp_of(dr, *nonneg[2]),
           sp_of(dr, *nonneg[3]), sp_of(dr, cases[4][0], cases[4][1])]
    with torch.no_grad():
        got = dr.embedding_lookup_sparse_multi(
            [va, ev, dense, mh, vb], sps, combiner="mean",
            adaptive_masks=[T(masks[0]), None, None, None, T(masks[4])])
    dr.status_check()
    wa, wb, ev2 = make(dr, D, H), make(dr, D, H), fresh()
    with torch.no_grad():
        parts = [dr.embedding_lookup_sparse(wa, sps[0], combiner="mean",
                                            adaptive_mask_tensor=T(masks[0])),
                 dr.embedding_lookup_sparse(ev2, sps[1], combiner="mean"),
                 dr.embedding_lookup_sparse(dense, sps[2], combiner="mean"),
                 dr.embedding_lookup_sparse(mh, sps[3], combiner="mean"),
                 dr.embedding_lookup_sparse(wb, sps[4], combiner="mean",
                                            adaptive_mask_tensor=T(masks[4]))]
    assert got.shape == (B, 5 * D)
    assert same(got, torch.cat(parts, 1))
    for a, b in ((va, wa), (vb, wb)):
        assert_same_ev(a.ev, b.ev)
    assert_same_ev(ev, ev2)
    want, _ = model_lookup(orc, H, ref.DictEV(D), cases[0][0], cases[0][1], masks[0])
    assert same(got[:, :D], want)


# ---------------------------------------------------------------------------
# 7. read-only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
def test_read_only_lookups_change_nothing(dr, orc, filtered):
    D = 16
    H = table(81, D)
    opt = (lambda: counter3(dr)) if filtered else (lambda: None)
    v, twin = make(dr, D, H, opt()), Twin(dr, orc, D, H, opt())
    model = ref.DictEV(D, filter_freq=3 if filtered else 0)
    ind, ids, w, _ = bags(82, True)
    warm = mask_of("parity", ids)
    for _ in range(4 if filtered else 1):       # odd ids get rows (a filter admits them in time)
        with torch.no_grad():
            dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), combiner="sum",
                                       adaptive_mask_tensor=T(warm))
            twin.lookup(ind, ids, warm, combiner="sum")
        model_lookup(orc, H, model, ind, ids, warm, combiner="sum")
    # the hash table moves on, so an EV row and a hash row differ
    for t in (v.hash_table, twin.hash):
        t.weight.mul_(2.0)
    H2 = (H * np.float32(2.0)).astype(np.float32)
    before = export_np(v.ev)
    size = int(v.ev.total_count()[0])
    assert size > 0
    mask = mask_of("random", ids, 6)            # names ids with a row and ids without
    with dr.read_only_lookups():
        got = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), spw_of(dr, ind, w),
                                         combiner="mean", adaptive_mask_tensor=T(mask))
        both = dr.embedding_lookup_sparse_multi([v, twin.ev], [sp_of(dr, ind, ids)] * 2,
                                                combiner="sum", adaptive_masks=[T(mask), None])
        tw = twin.lookup(ind, ids, mask, weights=w, combiner="mean")
    assert not got.requires_grad
    want, s = model_lookup(orc, H2, model, ind, ids, mask, weights=w, combiner="mean",
                           read_only=True)
    assert same(got, tw) and same(got, want)
    want_sum, _ = model_lookup(orc, H2, model, ind, ids, mask, combiner="sum", read_only=True)
    assert same(both[:, :D], want_sum)
    known = set(before[0].tolist())
    assert any(k in known for k in s["ev_keys"].tolist())
    assert any(k not in known for k in s["ev_keys"].tolist())
    for a, b in zip(before, export_np(v.ev)):
        assert same(a, b)
    assert int(v.ev.total_count()[0]) == size
    assert same(v.hash_table.weight, H2)
    assert not v.ev.pending_grads and not v.hash_table.pending_grads
    assert_same_ev(v.ev, twin.ev)
    dr.status_check()


# ---------------------------------------------------------------------------
# 8. supplied bucket rows
# ---------------------------------------------------------------------------
def test_supplied_hash_ev_ids_are_honoured_and_checked(dr, orc):
    D = 16
    H = table(91, D)
    v, twin, model = make(dr, D, H), Twin(dr, orc, D, H), ref.DictEV(D)
    ind, ids, _, _ = bags(92)
    rng = np.random.default_rng(93)
    u, inv = np.unique(ids, return_inverse=True)
    hrows = rng.integers(0, BUCKET, u.size)[inv].astype(np.int64)      # not the floor mod
    assert (hrows != ids % BUCKET).any()
    mask = mask_of("random", ids, 7)
    hs = sp_of(dr, ind, hrows)                                         # a SparseTensor, as sp_ids
    with torch.no_grad():
        got = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), combiner="mean",
                                         adaptive_mask_tensor=T(mask), hash_ev_ids=hs)
        tw = twin.lookup(ind, ids, mask, hash_rows=hrows, combiner="mean")
    want, _ = model_lookup(orc, H, model, ind, ids, mask, hash_rows=hrows)
    assert same(got, tw) and same(got, want)
    assert_same_ev(v.ev, twin.ev)
    # one bucket row out of range: an argument error that latches; row 0 is served, no fault
    bad = hrows.copy()
    k = int(np.flatnonzero(mask == 0)[0])
    bad[ids == ids[k]] = BUCKET
    k1 = int(np.flatnonzero((mask == 1) & (ids != ids[k]))[0])
    bad[ids == ids[k1]] = -1
    v2, model2 = make(dr, D, H), ref.DictEV(D)
    dr.set_validate(False)
    try:
        with torch.no_grad():
            got = dr.embedding_lookup_sparse(v2, sp_of(dr, ind, ids), combiner="mean",
                                             adaptive_mask_tensor=T(mask), hash_ev_ids=T(bad))
        with pytest.raises(dr.InvalidArgumentError):
            dr.status_check()
        dr.status_check()                                  # cleared
    finally:
        dr.set_validate(True)
    want, s = model_lookup(orc, H, model2, ind, ids, mask, hash_rows=bad)
    assert s["bad"] and same(got, want)
    assert same(v2.ev.sparse_read(T(np.array([ids[k1]])), read_only=True)[0], H[0])
    assert same(v2.hash_table.weight, H)


# ---------------------------------------------------------------------------
# 9. the C entries alone, with device counts below the capacity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", (16, 6, 260))
@pytest.mark.parametrize("mask_dtype", (np.uint8, np.int32, np.int64))
def test_c_entries_with_device_counts(dr, orc, D, mask_dtype):
    from deeprec_amd._lib import check, lib, stream_handle
    H = table(101, D)
    rng = np.random.default_rng(102)
    nnz, cap = 40, 40
    ids = rng.integers(0, NIDS, nnz).astype(np.int64)
    ids[5], ids[6] = ODD_IDS
    ids[20:30] = ids[:10]
    mask = mask_of("disagree", ids, 8).astype(mask_dtype)
    uids, idx, counts, m_u, h_u, _ = ref.per_id(orc, ids, mask, BUCKET)
    U = uids.size
    assert U < cap
    BIG = 1 << 40
    uniq = np.full(cap, BIG, np.int64)
    uniq[:U] = uids
    cnt = np.full(cap, 77, np.int32)
    cnt[:U] = counts
    st = stream_handle(torch.device(DEV))
    t_uniq, t_idx, t_cnt, t_U = T(uniq), T(idx.astype(np.int32)), T(cnt), T(np.array([U]))
    t_mask, t_H = T(mask), T(H)
    mask_u = torch.full((cap,), 9, dtype=torch.int32, device=DEV)
    hrow = torch.full((cap,), BIG, dtype=torch.int64, device=DEV)
    ev_keys = torch.full((cap,), BIG, dtype=torch.int64, device=DEV)
    ev_src = torch.full((cap,), 1 << 30, dtype=torch.int32, device=DEV)
    ev_cnt = torch.full((cap,), 77, dtype=torch.int32, device=DEV)
    Ue = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    dflt = torch.full((cap, D), float("nan"), dtype=torch.float32, device=DEV)
    wsb = lib().dr_adaptive_split_workspace_size(nnz)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    check(lib().dr_adaptive_split(t_uniq.data_ptr(), t_idx.data_ptr(), nnz, t_U.data_ptr(),
                                  t_mask.data_ptr(), mask.itemsize, None, BUCKET, t_H.data_ptr(), D,
                                  t_cnt.data_ptr(), mask_u.data_ptr(), hrow.data_ptr(),
                                  ev_keys.data_ptr(), ev_src.data_ptr(), ev_cnt.data_ptr(),
                                  Ue.data_ptr(), dflt.data_ptr(), ws.data_ptr(), wsb, st))
    dr.status_check()
    src = np.flatnonzero(m_u)
    n_ev = src.size
    assert 0 < n_ev < U and int(Ue.item()) == n_ev
    assert np.array_equal(mask_u[:U].cpu().numpy(), m_u.astype(np.int32))
    assert np.array_equal(hrow[:U].cpu().numpy(), h_u)
    assert np.array_equal(ev_keys[:n_ev].cpu().numpy(), uids[src])
    assert np.array_equal(ev_src[:n_ev].cpu().numpy(), src.astype(np.int32))
    assert np.array_equal(ev_cnt[:n_ev].cpu().numpy(), counts[src])
    assert same(dflt[:n_ev], H[h_u[src]])
    # nothing at or past the counts was written
    assert (mask_u[U:] == 9).all() and (hrow[U:] == BIG).all()
    assert (ev_keys[n_ev:] == BIG).all() and (ev_src[n_ev:] == 1 << 30).all()
    assert (ev_cnt[n_ev:] == 77).all() and torch.isnan(dflt[n_ev:]).all()
    # merge: every second EV id resolved to a row, the others "serve the default"
    ev_rows = np.full(cap, BIG, np.int64)
    ev_rows[:n_ev] = np.where(np.arange(n_ev) % 2 == 0, 1000 + np.arange(n_ev),
                              -(np.arange(n_ev) + 1))
    rows_u = torch.full((cap,), BIG, dtype=torch.int64, device=DEV)
    t_rows = T(ev_rows)
    check(lib().dr_adaptive_merge(mask_u.data_ptr(), hrow.data_ptr(), ev_src.data_ptr(),
                                  t_rows.data_ptr(), cap, t_U.data_ptr(), Ue.data_ptr(),
                                  rows_u.data_ptr(), st))
    want = -(h_u + 1)
    want[src[::2]] = 1000 + np.arange(n_ev)[::2]
    assert np.array_equal(rows_u[:U].cpu().numpy(), want) and (rows_u[U:] == BIG).all()
    # grad: NaN rows past the count are never read as rows
    gu = np.full((cap, D), np.nan, np.float32)
    gu[:U] = rng.standard_normal((U, D)).astype(np.float32)
    t_gu = T(gu)
    ev_val = torch.full((cap, D), 7.0, dtype=torch.float32, device=DEV)
    hidx = torch.full((cap,), BIG, dtype=torch.int64, device=DEV)
    check(lib().dr_adaptive_grad(t_gu.data_ptr(), D, mask_u.data_ptr(), hrow.data_ptr(),
                                 ev_src.data_ptr(), cap, t_U.data_ptr(), Ue.data_ptr(),
                                 ev_val.data_ptr(), hidx.data_ptr(), st))
    dr.status_check()
    ek, evv, hi, _ = ref.split(gu[:U], m_u, h_u, uids)
    assert same(ev_val[:n_ev], evv) and (ev_val[n_ev:] == 7.0).all()
    assert np.array_equal(hidx[:U].cpu().numpy(), hi) and (hidx[U:] == -1).all()
    assert same(t_gu, gu)


# ---------------------------------------------------------------------------
# 10. safe_embedding_lookup_sparse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("default_id", [None, 3])
def test_safe_lookup_prunes_and_fills(dr, orc, default_id):
    D = 16
    H = table(111, D)
    ind, ids, w, lens = bags(112, True)
    ids = np.where(ids < 0, 3, ids)                      # (a negative id would be pruned anyway)
    ids[::5] = -1 - ids[::5]                             # ids < 0 are pruned
    width = int(ind[:, 1].max()) + 1
    mask = mask_of("random", np.abs(ids), 9)
    mask[ids < 0] = 1 - mask[ids < 0]                    # pruned positions must not matter
    for weights in (None, w):
        for combiner in ("mean", "sum"):
            v, model = make(dr, D, H), ref.DictEV(D)
            with torch.no_grad():
                got = dr.safe_embedding_lookup_sparse(
                    v, sp_of(dr, ind, ids), spw_of(dr, ind, weights), combiner=combiner,
                    default_id=default_id, adaptive_mask_tensor=T(mask))
            pi, pv, pw, empty = orc.prune_and_fill(ind, ids, (B, width), weights, combiner,
                                                   default_id, True)
            # the mask follows its id through the prune; a filled default id takes mask 0
            kept = {(int(r), int(c)): int(m) for (r, c), m in zip(ind.tolist(), mask.tolist())}
            filled = set(np.flatnonzero(empty).tolist())
            pm = np.array([0 if int(r) in filled else kept[(int(r), int(c))]
                           for r, c in pi.tolist()], np.int64)
            want, s = model_lookup(orc, H, model, pi, pv, pm, weights=pw, combiner=combiner)
            if default_id is None:
                want[empty] = 0.0
            assert same(got, want), (combiner, weights is None, default_id)
            assert np.array_equal(export_np(v.ev)[0], np.sort(s["ev_keys"]))
    assert empty.any()
    dr.status_check()


def test_the_sharded_engines_refuse_the_variable(dr):
    from deeprec_amd import sharded
    v = make(dr, 16, table(121, 16))
    for ctor in (lambda: sharded.HipLocal([v], DEV),
                 lambda: sharded.ShardedLookup([v], 1, 0, B, DEV),
                 lambda: sharded.NativeShardedLookup(None, [v], DEV),
                 lambda: sharded.ReduceScatterShardedLookup([v], 1, 0, B, DEV),
                 lambda: sharded.XgmiShardedLookup([v], 1, 0, B, DEV)):
        with pytest.raises(dr.InvalidArgumentError, match="AdaptiveEmbeddingVariable"):
            ctor()
    # the variable is in the registry that reset_registry() clears: asked for again, it is itself
    import deeprec_amd.kv_variable_ops as kv
    assert kv._EV_REGISTRY[v.name] is v
    assert dr.get_adaptive_embedding_variable(v.name, 16, BUCKET, device=DEV) is v
