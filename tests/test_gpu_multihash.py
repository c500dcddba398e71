"""MultiHashVariable ("Q-R") on the GPU: the fused pooled lookup, the unpooled
lookup and the gradient split against tests/multihash_ref.py (numpy + the CPU
oracle) and against the existing lookup over a DenseTable that holds the
materialised rows.  Every comparison is bit equality (NaNs must coincide).

Shapes are the smallest at which each piece can go wrong: B = 64, Q = 7 rows,
R = 5 rows (Q != R pins the index rule), ids in [0, 49); row widths 4, 6, 16,
128, 260 (vector / scalar layouts, one and several chunks per lane) and
concat as 8 + 4 and 4 + 6; bag lengths 0, 1, 2, 7, 8, 9, 10, 16, 17, 33 (every
first-chunk size of the association order, both sides of the num < 10 rule,
several chunks of 8) with repeats inside a bag."""
import ctypes as C

import numpy as np
import pytest
import torch

import multihash_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, Q, R = 64, 7, 5
NIDS = Q * Q
LENS = [0, 1, 2, 7, 8, 9, 10, 16, 17, 33]
SHAPES = [("add", d, d) for d in (4, 6, 16, 128, 260)] + \
         [("mul", d, d) for d in (4, 6, 16, 128, 260)] + [("concat", 8, 4), ("concat", 4, 6)]
COMBINERS = ("sum", "mean", "sqrtn")
_N = [0]


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    from deeprec_amd import get_multihash_variable  # noqa: F401  (the feature under test)
    deeprec_amd.load()
    deeprec_amd.set_validate(True)
    assert torch.cuda.is_available()
    return deeprec_amd


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), device=DEV, dtype=dtype)


def same(a, b):
    """Bit equality of two fp32 arrays, NaNs at the same places."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def tables(seed, dq, dr_):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((Q, dq)).astype(np.float32),
            rng.standard_normal((R, dr_)).astype(np.float32))


def make(dr, op, Qt, Rt):
    _N[0] += 1
    return dr.get_multihash_variable("mhv%d" % _N[0], [list(Qt.shape), list(Rt.shape)],
                                     operation=op, initializer=[T(Qt), T(Rt)], device=DEV)


_CASES = {}


def bags(seed, weighted=False):
    """indices [nnz, 2], ids [nnz], weights: 64 bags whose lengths go through
    LENS (then random ones), ids in [0, 49) with repeats inside a bag."""
    key = (seed, weighted)
    if key not in _CASES:
        rng = np.random.default_rng(seed)
        lens = np.array(LENS + list(rng.choice(LENS, B - len(LENS))))
        rng.shuffle(lens)
        rows = np.repeat(np.arange(B), lens)
        cols = np.concatenate([np.arange(n) for n in lens])
        ind = np.stack([rows, cols], 1).astype(np.int64)
        ids = rng.integers(0, NIDS, rows.size).astype(np.int64)
        for b in np.flatnonzero(lens >= 2):             # a repeat inside every longer bag
            k0 = int(np.searchsorted(rows, b))
            ids[k0 + 1] = ids[k0]
        w = rng.uniform(0.25, 2.0, rows.size).astype(np.float32) if weighted else None
        _CASES[key] = (ind, ids, w, lens)
    return _CASES[key]


def sp_of(dr, ind, ids, width=None):
    width = int(ind[:, 1].max()) + 1 if width is None else width
    return dr.SparseTensor(T(ind), T(ids), (B, width))


def spw_of(dr, ind, w):
    return None if w is None else dr.SparseTensor(T(ind), T(w), (B, int(ind[:, 1].max()) + 1))


# ---------------------------------------------------------------------------
# 1. pooled forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("op,dq,dr_", SHAPES)
def test_pooled_forward(dr, orc, op, dq, dr_, combiner):
    Qt, Rt = tables(dq * 31 + dr_, dq, dr_)
    v = make(dr, op, Qt, Rt)
    dense = dr.DenseTable(T(ref.materialize(orc, Qt, Rt, op, NIDS)))
    for weighted in (False, True):
        ind, ids, w, lens = bags(5, weighted)
        assert 0 in lens            # (weighted mean / sqrtn: the NaN of an empty bag)
        with torch.no_grad():
            got = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), spw_of(dr, ind, w),
                                             combiner=combiner)
            mat = dr.embedding_lookup_sparse(dense, sp_of(dr, ind, ids), spw_of(dr, ind, w),
                                             combiner=combiner)
        want = ref.lookup_sparse(orc, Qt, Rt, op, ind, ids, B, weights=w, combiner=combiner)
        assert got.shape == (B, v.dim)
        assert same(got, want), (op, dq, dr_, combiner, weighted)
        assert same(got, mat), (op, dq, dr_, combiner, weighted)
        if weighted and combiner != "sum":
            assert np.isnan(want[lens == 0]).all() and not np.isnan(want[lens > 0]).any()
    dr.status_check()
    assert same(v.val_list[0].weight, Qt) and same(v.val_list[1].weight, Rt)


@pytest.mark.parametrize("op,dq,dr_", SHAPES)
def test_onehot_route(dr, orc, op, dq, dr_):
    Qt, Rt = tables(dq * 17 + dr_, dq, dr_)
    v = make(dr, op, Qt, Rt)
    ids = np.random.default_rng(3).integers(0, NIDS, B).astype(np.int64)
    ind = np.stack([np.arange(B), np.zeros(B, np.int64)], 1).astype(np.int64)
    sp = dr.SparseTensor(T(ind), T(ids), (B, 1))
    dense = dr.DenseTable(T(ref.materialize(orc, Qt, Rt, op, NIDS)))
    for combiner in COMBINERS:
        with torch.no_grad():
            got = dr.embedding_lookup_sparse(v, sp, combiner=combiner)
            mat = dr.embedding_lookup_sparse(dense, sp, combiner=combiner)
        want = ref.lookup_sparse(orc, Qt, Rt, op, ind, ids, B, combiner=combiner)
        assert same(got, want) and same(got, mat), (op, dq, dr_, combiner)
        assert same(got, ref.rows(orc, Qt, Rt, op, ids))      # a bag of one id is the row
    dr.status_check()


@pytest.mark.parametrize("default_id", [None, 3])
@pytest.mark.parametrize("op,dq,dr_", [("add", 16, 16), ("mul", 6, 6), ("concat", 8, 4)])
def test_safe_lookup_prunes_and_fills(dr, orc, op, dq, dr_, default_id):
    Qt, Rt = tables(11, dq, dr_)
    v = make(dr, op, Qt, Rt)
    ind, ids, w, lens = bags(6, True)
    ids = ids.copy()
    ids[::5] = -1 - ids[::5]                         # ids < 0 are pruned
    width = int(ind[:, 1].max()) + 1
    for weights in (None, w):
        for combiner in ("mean", "sum"):
            with torch.no_grad():
                got = dr.safe_embedding_lookup_sparse(
                    v, sp_of(dr, ind, ids), spw_of(dr, ind, weights), combiner=combiner,
                    default_id=default_id)
            pi, pv, pw, empty = orc.prune_and_fill(ind, ids, (B, width), weights, combiner,
                                                   default_id, True)
            want = ref.lookup_sparse(orc, Qt, Rt, op, pi, pv, B, weights=pw, combiner=combiner)
            if default_id is None:
                want[empty] = 0.0
            assert same(got, want), (op, combiner, weights is None, default_id)
    dr.status_check()


# ---------------------------------------------------------------------------
# 2. grouped calls
# ---------------------------------------------------------------------------
def ev_with_rows(dr, D, seed):
    _N[0] += 1
    ev = dr.EmbeddingVariable("mhv_ev%d" % _N[0], D, 0.25)
    rng = np.random.default_rng(seed)
    keys = np.arange(0, NIDS, 2, dtype=np.int64)      # the other ids are created by the lookup
    ev.insert(T(keys), T(rng.standard_normal((keys.size, D)).astype(np.float32)))
    return ev


def test_multi_call_mixes_multihash_dense_and_ev_features(dr, orc):
    QA, RA = tables(21, 16, 16)
    QB, RB = tables(22, 8, 4)
    va, vb = make(dr, "mul", QA, RA), make(dr, "concat", QB, RB)
    dt = np.random.default_rng(23).standard_normal((NIDS, 16)).astype(np.float32)
    dense = dr.DenseTable(T(dt))
    ev, ev2 = ev_with_rows(dr, 16, 24), ev_with_rows(dr, 16, 24)
    cases = [bags(s) for s in (31, 32, 33, 34, 35)]
    sps = [sp_of(dr, c[0], c[1]) for c in cases]
    with torch.no_grad():
        got = dr.embedding_lookup_sparse_multi([va, dense, vb, va, ev], sps, combiner="mean")
        plain = dr.embedding_lookup_sparse_multi([dense, ev2], [sps[1], sps[4]], combiner="mean")
    dr.status_check()
    parts = [ref.lookup_sparse(orc, QA, RA, "mul", cases[0][0], cases[0][1], B),
             orc.embedding_lookup_sparse(dt, cases[1][0], cases[1][1], B),
             ref.lookup_sparse(orc, QB, RB, "concat", cases[2][0], cases[2][1], B),
             ref.lookup_sparse(orc, QA, RA, "mul", cases[3][0], cases[3][1], B),
             plain[:, 16:].cpu().numpy()]
    assert got.shape == (B, 16 + 16 + 12 + 16 + 16)
    assert same(got, np.concatenate(parts, 1))
    assert same(plain[:, :16], parts[1])
    for a, b in zip(ev.export(), ev2.export()):
        assert torch.equal(a, b)


def test_33_features_take_two_launches(dr, orc):
    vs = [make(dr, op, *tables(40 + i, 4, 4)) for i, op in enumerate(("add", "mul", "concat"))]
    rng = np.random.default_rng(41)
    ids = rng.integers(0, NIDS, (33, B)).astype(np.int64)
    ind = np.stack([np.arange(B), np.zeros(B, np.int64)], 1).astype(np.int64)
    params = [vs[t % 3] for t in range(33)]
    with torch.no_grad():
        got = dr.embedding_lookup_sparse_multi(
            params, [dr.SparseTensor(T(ind), T(ids[t]), (B, 1)) for t in range(33)],
            combiner="sum")
    dr.status_check()
    want = np.concatenate([ref.rows(orc, p.val_list[0].weight.cpu().numpy(),
                                    p.val_list[1].weight.cpu().numpy(), p.operation, ids[t])
                           for t, p in enumerate(params)], 1)
    assert got.shape == (B, 11 * (4 + 4 + 8)) and same(got, want)


# ---------------------------------------------------------------------------
# 3. unpooled, out of range
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("op,dq,dr_", SHAPES)
def test_unpooled_lookup(dr, orc, op, dq, dr_):
    Qt, Rt = tables(50 + dq, dq, dr_)
    v = make(dr, op, Qt, Rt)
    rng = np.random.default_rng(51)
    for shape in ((37,), (5, 9)):
        ids = rng.integers(0, NIDS, shape).astype(np.int64)
        got = dr.embedding_lookup(v, T(ids))
        assert tuple(got.shape) == shape + (v.dim,)
        assert same(got, ref.lookup(orc, Qt, Rt, op, ids))
    dr.status_check()


@pytest.mark.parametrize("op,dq,dr_", [("add", 16, 16), ("mul", 6, 6), ("concat", 8, 4)])
def test_out_of_range_ids_are_zero_rows_and_latch(dr, orc, op, dq, dr_):
    Qt, Rt = tables(60, dq, dr_)
    v = make(dr, op, Qt, Rt)
    ind, ids, _, lens = bags(7)
    ids = ids.copy()
    bad = np.flatnonzero(lens >= 7)[:2]
    k = [int(np.searchsorted(ind[:, 0], b)) + 2 for b in bad]
    ids[k[0]], ids[k[1]] = Q * Q, -1
    dr.set_validate(False)
    try:
        with torch.no_grad():
            got = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), combiner="mean")
        with pytest.raises(dr.InvalidArgumentError):
            dr.status_check()
        dr.status_check()                              # cleared
        flat = dr.embedding_lookup(v, T(np.array([3, Q * Q, -1, 48], np.int64)))
        with pytest.raises(dr.InvalidArgumentError):
            dr.status_check()
    finally:
        dr.set_validate(True)
    want = ref.lookup_sparse(orc, Qt, Rt, op, ind, ids, B, combiner="mean")
    assert same(got, want)
    frows = ref.rows(orc, Qt, Rt, op, [3, Q * Q, -1, 48])
    assert not frows[1].any() and not frows[2].any() and frows[0].any()
    assert same(flat, frows)
    assert same(v.val_list[0].weight, Qt) and same(v.val_list[1].weight, Rt)


# ---------------------------------------------------------------------------
# 4. gradient
# ---------------------------------------------------------------------------
def check_slices(sl, idx, val):
    U = idx.size
    assert sl.num_valid is not None and int(sl.num_valid.item()) == U
    n = sl.indices.numel()
    assert n >= U and tuple(sl.values.shape) == (n, val.shape[1])
    assert np.array_equal(sl.indices[:U].cpu().numpy(), idx)
    assert same(sl.values[:U], val)
    # past the device count: index -1 and zero rows (skipped like seg < 0)
    assert (sl.indices[U:] == -1).all() and not sl.values[U:].any()


def has_repeats(ids):
    """>= 10 distinct ids share a q row and >= 10 share an r row."""
    u = np.unique(ids)
    q, r, _ = ref.index(u, Q, R)
    return (u.size - np.unique(q).size >= 10) and (u.size - np.unique(r).size >= 10)


@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("op,dq,dr_", [("add", 16, 16), ("mul", 16, 16), ("concat", 8, 4),
                                       ("add", 6, 6), ("mul", 6, 6), ("concat", 4, 6),
                                       ("mul", 260, 260)])
def test_gradient_slices(dr, orc, op, dq, dr_, combiner):
    Qt, Rt = tables(70, dq, dr_)
    rng = np.random.default_rng(71)
    for weighted in (False, True):
        v = make(dr, op, Qt, Rt)
        ind, ids, w, _ = bags(8, weighted)
        ind2, ids2, _, _ = bags(9)
        assert np.unique(ids).size >= 20 and has_repeats(ids) and has_repeats(ids2)
        g = rng.standard_normal((B, 2 * v.dim)).astype(np.float32)
        out = dr.embedding_lookup_sparse_multi if not weighted else None
        if weighted:      # one weighted feature
            res = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), spw_of(dr, ind, w),
                                             combiner=combiner)
            res.backward(T(g[:, :v.dim]))
            wants = [ref.lookup_sparse_grad(orc, Qt, Rt, op, ind, ids, B, g[:, :v.dim],
                                            weights=w, combiner=combiner)]
        else:             # two features over the same variable in one call
            res = out([v, v], [sp_of(dr, ind, ids), sp_of(dr, ind2, ids2)], combiner=combiner)
            res.backward(T(g))
            wants = [ref.lookup_sparse_grad(orc, Qt, Rt, op, ind, ids, B, g[:, :v.dim],
                                            combiner=combiner),
                     ref.lookup_sparse_grad(orc, Qt, Rt, op, ind2, ids2, B, g[:, v.dim:],
                                            combiner=combiner)]
        dr.status_check()
        tq, tr = v.val_list
        assert len(tq.pending_grads) == len(wants) and len(tr.pending_grads) == len(wants)
        for sq, sr, (uids, gu, qi, qv, ri, rv) in zip(tq.pending_grads, tr.pending_grads, wants):
            assert np.unique(qi).size < qi.size and np.unique(ri).size < ri.size   # repeats
            check_slices(sq, qi, qv)
            check_slices(sr, ri, rv)
        # the factor rows of mul are the tables as they stand: nothing was updated
        assert same(tq.weight, Qt) and same(tr.weight, Rt)


@pytest.mark.parametrize("opt_name", ["sgd", "adagrad"])
@pytest.mark.parametrize("op", ["add", "mul"])
def test_five_training_steps_equal_the_twin_tables(dr, orc, op, opt_name):
    D = 16
    Qt, Rt = tables(80, D, D)
    v = make(dr, op, Qt, Rt)
    twins = [dr.DenseTable(T(Qt)), dr.DenseTable(T(Rt))]

    def opt():
        return dr.GradientDescentOptimizer(0.05) if opt_name == "sgd" else \
            dr.AdagradOptimizer(0.05, initial_accumulator_value=0.1)
    o1, o2 = opt(), opt()
    rng = np.random.default_rng(81)
    for step in range(5):
        ind, ids, w, _ = bags(90 + step, step % 2 == 1)
        g = rng.standard_normal((B, D)).astype(np.float32)
        res = dr.embedding_lookup_sparse(v, sp_of(dr, ind, ids), spw_of(dr, ind, w),
                                         combiner="mean")
        # the twins' tables, before the update, feed the reference's slices
        tq, tr = (t.weight.cpu().numpy() for t in twins)
        assert same(res, ref.lookup_sparse(orc, tq, tr, op, ind, ids, B, weights=w))
        res.backward(T(g))
        _, _, qi, qv, ri, rv = ref.lookup_sparse_grad(orc, tq, tr, op, ind, ids, B, g, weights=w)
        twins[0].pending_grads.append(dr.IndexedSlices(T(qv), T(qi)))
        twins[1].pending_grads.append(dr.IndexedSlices(T(rv), T(ri)))
        o1.apply_gradients([v], global_step=step)        # the variable itself in var_list
        o2.apply_gradients(twins, global_step=step)
        dr.status_check()
        assert not v.val_list[0].pending_grads and not v.val_list[1].pending_grads
        for mine, twin in zip(v.val_list, twins):
            assert same(mine.weight, twin.weight), (op, opt_name, step)
    assert not same(v.val_list[0].weight, Qt) and not same(v.val_list[1].weight, Rt)


# ---------------------------------------------------------------------------
# 5. the C entries alone
# ---------------------------------------------------------------------------
def _targs(Qt, Rt, op):
    from deeprec_amd._lib import MHV_OPERATIONS
    tq, tr = T(Qt), T(Rt)
    return (tq, tr), [tq.data_ptr(), Qt.shape[0], Qt.shape[1], tr.data_ptr(), Rt.shape[0],
                      Rt.shape[1], MHV_OPERATIONS[op]]


@pytest.mark.parametrize("op,dq,dr_", [("add", 16, 16), ("mul", 6, 6), ("concat", 8, 4),
                                       ("concat", 4, 6)])
def test_c_entries_with_a_device_count(dr, orc, op, dq, dr_):
    from deeprec_amd._lib import COMBINERS as CODES, DrMhvDesc, check, lib, stream_handle
    Qt, Rt = tables(100, dq, dr_)
    keep, targs = _targs(Qt, Rt, op)
    dim = ref.dim_of(Qt, Rt, op)
    rng = np.random.default_rng(101)
    n, m = 40, 25
    ids = rng.integers(0, NIDS, n).astype(np.int64)
    ids[3] = Q * Q                                              # out of range, below the count
    ids[30] = -5                                                # ... and past it: not looked at
    tids, ndev = T(ids), T(np.array([m], np.int64))
    st = stream_handle(torch.device(DEV))
    # gather: rows past the count are left as they were
    out = torch.full((n, dim), 7.0, dtype=torch.float32, device=DEV)
    check(lib().dr_mhv_gather(*targs, tids.data_ptr(), n, ndev.data_ptr(), out.data_ptr(), st))
    with pytest.raises(dr.InvalidArgumentError):
        dr.status_check()                                       # ids[3]
    want = ref.rows(orc, Qt, Rt, op, ids)
    assert same(out[:m], want[:m]) and (out[m:] == 7.0).all() and not want[3].any()
    ids[3] = 4
    tids = T(ids)
    check(lib().dr_mhv_gather(*targs, tids.data_ptr(), n, None, out.data_ptr(), st))
    with pytest.raises(dr.InvalidArgumentError):
        dr.status_check()                                       # ids[30], now inside n
    assert same(out, ref.rows(orc, Qt, Rt, op, ids))
    # grad: past the count index -1 and zero rows
    ids[30] = 12
    ids[5] = Q * Q + 1
    tids = T(ids)
    gu = rng.standard_normal((n, dim)).astype(np.float32)
    tgu = T(gu)
    qi = torch.full((n,), 99, dtype=torch.int64, device=DEV)
    ri = torch.full((n,), 99, dtype=torch.int64, device=DEV)
    qv = torch.full((n, dq), 7.0, dtype=torch.float32, device=DEV)
    rv = qv if op == "add" else torch.full((n, dr_), 7.0, dtype=torch.float32, device=DEV)
    check(lib().dr_mhv_grad(*targs, tids.data_ptr(), tgu.data_ptr(), n, ndev.data_ptr(),
                            qi.data_ptr(), ri.data_ptr(), qv.data_ptr(), rv.data_ptr(), st))
    dr.status_check()
    wqi, wqv, wri, wrv = ref.split(Qt, Rt, op, ids[:m], gu[:m])
    assert wqi[5] == -1 and wri[5] == -1 and not wqv[5].any() and not wrv[5].any()
    assert np.array_equal(qi[:m].cpu().numpy(), wqi) and np.array_equal(ri[:m].cpu().numpy(), wri)
    assert same(qv[:m], wqv) and same(rv[:m], wrv)
    assert (qi[m:] == -1).all() and (ri[m:] == -1).all()
    assert not qv[m:].any() and not rv[m:].any()
    # the pooled entry: two descriptors, one with bag offsets and weights, one one-hot
    ind, bids, w, _ = bags(102, True)
    off = T(np.concatenate([[0], np.cumsum(np.bincount(ind[:, 0], minlength=B))]), torch.int32)
    tb, tw = T(bids), T(w)
    hot = T(rng.integers(0, NIDS, B).astype(np.int64))
    out = torch.full((B, 2 * dim + 3), 7.0, dtype=torch.float32, device=DEV)
    descs = (DrMhvDesc * 2)()
    for d, col in zip(descs, (0, dim)):
        (d.q_table, d.q_rows, d.q_dim, d.r_table, d.r_rows, d.r_dim, d.operation) = targs
        d.out, d.out_stride = out.data_ptr() + 4 * col, out.shape[1]
    descs[0].ids, descs[0].bag_off, descs[0].weights = tb.data_ptr(), off.data_ptr(), tw.data_ptr()
    descs[0].combiner = CODES["sqrtn"]
    descs[1].ids, descs[1].combiner = hot.data_ptr(), CODES["mean"]
    check(lib().dr_mhv_lookup_sparse_grouped(descs, 2, B, st))
    dr.status_check()
    assert same(out[:, :dim], ref.lookup_sparse(orc, Qt, Rt, op, ind, bids, B, weights=w,
                                                combiner="sqrtn"))
    assert same(out[:, dim:2 * dim], ref.rows(orc, Qt, Rt, op, hot.cpu().numpy()))
    assert (out[:, 2 * dim:] == 7.0).all()                       # nothing past the columns
    del keep


# ---------------------------------------------------------------------------
# 6. stream capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("op,dq,dr_", [("add", 128, 128), ("concat", 8, 4)])
def test_captured_forward_replays_with_new_ids(dr, orc, op, dq, dr_):
    Qt, Rt = tables(110, dq, dr_)
    v = make(dr, op, Qt, Rt)
    ind, ids, _, _ = bags(111)
    hot_ind = np.stack([np.arange(B), np.zeros(B, np.int64)], 1).astype(np.int64)
    rng = np.random.default_rng(112)
    hot = rng.integers(0, NIDS, B).astype(np.int64)
    sp, sph = sp_of(dr, ind, ids), dr.SparseTensor(T(hot_ind), T(hot), (B, 1))
    with torch.no_grad():
        eager = dr.embedding_lookup_sparse_multi([v, v], [sp, sph], combiner="mean")   # warm-up
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                  # one stream, no parallel branches
            out = dr.embedding_lookup_sparse_multi([v, v], [sp, sph], combiner="mean")
    for _ in range(2):
        ids = rng.integers(0, NIDS, ids.size).astype(np.int64)
        hot = rng.integers(0, NIDS, B).astype(np.int64)
        sp.values.copy_(T(ids))                    # the ids buffers rewritten in place
        sph.values.copy_(T(hot))
        g.replay()
        torch.cuda.synchronize()
        dr.status_check()
        with torch.no_grad():
            eager = dr.embedding_lookup_sparse_multi([v, v], [sp, sph], combiner="mean")
        assert same(out, eager)
        assert same(out[:, :v.dim], ref.lookup_sparse(orc, Qt, Rt, op, ind, ids, B))
        assert same(out[:, v.dim:], ref.rows(orc, Qt, Rt, op, hot))


# ---------------------------------------------------------------------------
# 7. what is refused
# ---------------------------------------------------------------------------
def test_refusals(dr):
    Qt, Rt = tables(120, 16, 16)
    v = make(dr, "add", Qt, Rt)
    ind, ids, _, _ = bags(121)
    sp = sp_of(dr, ind, ids)
    with pytest.raises(dr.InvalidArgumentError, match="max_norm"):
        dr.embedding_lookup_sparse(v, sp, combiner="sum", max_norm=1.0)
    with pytest.raises(dr.InvalidArgumentError, match="max_norm"):
        dr.embedding_lookup_sparse_multi([v], [sp], max_norm=1.0)
    with pytest.raises(dr.InvalidArgumentError, match="max_norm"):
        dr.embedding_lookup(v, T(ids), max_norm=1.0)
    with pytest.raises(dr.InvalidArgumentError, match="tile"):
        dr.embedding_lookup_sparse(v, sp, combiner="tile")
    with pytest.raises(dr.InvalidArgumentError, match="embedding_stack"):
        from deeprec_amd.embedding_ops import embedding_stack
        embedding_stack(torch.zeros((B, 16), device=DEV), [v], [sp])
    with pytest.raises(TypeError, match="MultiHashVariable"):
        dr.fused_embedding_lookup_sparse(v, sp, combiner="sum")
    with pytest.raises(TypeError, match="partition"):
        dr.embedding_lookup_sparse([v, v], sp, combiner="sum")
    with pytest.raises(TypeError, match="partition"):
        dr.embedding_lookup([v, v], T(ids))
    from deeprec_amd import sharded
    for ctor in (lambda: sharded.HipLocal([v], DEV),
                 lambda: sharded.ShardedLookup([v], 1, 0, B, DEV),
                 lambda: sharded.NativeShardedLookup(None, [v], DEV),
                 lambda: sharded.ReduceScatterShardedLookup([v], 1, 0, B, DEV),
                 lambda: sharded.XgmiShardedLookup([v], 1, 0, B, DEV)):
        with pytest.raises(TypeError, match="MultiHashVariable"):
            ctor()
    assert not v.val_list[0].pending_grads and not v.val_list[1].pending_grads
    dr.status_check()


def test_read_only_lookups_is_the_same_lookup(dr, orc):
    Qt, Rt = tables(130, 16, 16)
    v = make(dr, "mul", Qt, Rt)
    ev = ev_with_rows(dr, 16, 131)
    before = ev.export()
    ind, ids, _, _ = bags(132)
    sp = sp_of(dr, ind, ids)
    with dr.read_only_lookups(), torch.no_grad():
        alone = dr.embedding_lookup_sparse(v, sp, combiner="sqrtn")
        both = dr.embedding_lookup_sparse_multi([ev, v], [sp, sp], combiner="sqrtn")
    want = ref.lookup_sparse(orc, Qt, Rt, "mul", ind, ids, B, combiner="sqrtn")
    assert same(alone, want) and same(both[:, 16:], want)
    for a, b in zip(before, ev.export()):       # no key was created
        assert torch.equal(a, b)
    dr.status_check()
