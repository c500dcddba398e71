"""GPU: the HBM + host-DRAM tier of an EmbeddingVariable.

The contract is transparency: a tiered EV with any budget, demoted at any
moments, is observably equal to an untiered, unbudgeted twin that saw the same
calls -- bit-equal lookup outputs at every step, bit-equal export() of the
primary and of every slot EV, byte-equal checkpoint bundles.  Every test here
is a form of that sentence, so no tolerance appears anywhere.

capacity=1 (1 024 rows / 2 048 slots), dim 8, keys from ev_lifecycle.universe
(the four special keys, clustered groups whose probe chains wrap the table
end); values and gradients are multiples of 0.5, exact in bf16 too.
"""
import ctypes as C
import filecmp

import numpy as np
import pytest
import torch

import ev_lifecycle as L
import host_tier_walk as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIM = L.DIM
I64MAX = np.iinfo(np.int64).max
TORCH_DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float64": torch.float64}


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    return deeprec_amd


@pytest.fixture(scope="module")
def uni():
    return L.universe(5)


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def bits(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy()
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def snap(ev):
    k, v, ve, fr = ev.export()
    return k.cpu().numpy(), bits(v), ve.cpu().numpy(), fr.cpu().numpy()


def same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, i, x.shape, y.shape)
        assert np.array_equal(x, y), "%s: field %d differs, first at %s" % (
            what, i, np.argwhere(x != y)[0].tolist())


_N = [0]


def make(dr, tiered, dtype="float32", policy="lru", filter_freq=0, max_keys=W.BUDGET,
         stl=W.STEPS_TO_LIVE, dim=DIM, **kw):
    """A tiered EV, or its twin: untiered and unbudgeted, otherwise the same."""
    _N[0] += 1
    evict = dr.KeyBudgetEvict(max_keys, policy, steps_to_live=stl) if tiered \
        else dr.GlobalStepEvict(stl)
    opt = dr.EmbeddingVariableOption(
        evict_option=evict,
        filter_option=dr.CounterFilter(filter_freq) if filter_freq else None,
        storage_option=dr.StorageOption(dr.StorageType.HBM_DRAM) if tiered else None)
    kw.setdefault("capacity", 1)
    return dr.EmbeddingVariable("tier_%d_%s" % (_N[0], "a" if tiered else "b"), dim, L.DEFAULT,
                                ev_option=opt, device=DEV, value_dtype=TORCH_DT[dtype], **kw)


def tier_state(ev):
    """The host tier's content (keys ascending), host numpy."""
    with ev._lock:
        k, vals, ve, fr, cm = ev._tier_export()
    return [k, ve, fr, cm] + [v for v in vals if v is not None]


def train(dr, opt, ev, keys, step, seed=0, dtype="float32"):
    """One step on `ev`: the lookup of `keys` (duplicates and all), then SGD /
    Adagrad on the distinct keys with global_step = step.  A float64 EV trains
    by upsert of the step computed on the host (the applies take float rows)."""
    out = ev.sparse_read(T(keys))
    u, first = np.unique(keys, return_index=True)
    g = W.grads(seed, step, u.size)
    if dtype == "float64":
        new = out.cpu().numpy()[first] - L.LR * g.astype(np.float64)
        ev.upsert(T(u), T(new), T(np.full(u.size, step, np.int64)))
    else:
        ev.pending_grads.append(dr.IndexedSlices(T(g), T(u)))
        opt.apply_gradients([ev], global_step=step)
    return bits(out)


# ---------------------------------------------------------------------------
# 1. dr_ev_missing_keys
# ---------------------------------------------------------------------------
def missing(dr, evs, keys, n_dev=None):
    T_ = len(evs)
    flat = T(np.concatenate(keys)) if sum(k.size for k in keys) else \
        torch.empty(0, dtype=torch.int64, device=DEV)
    koff = np.concatenate([[0], np.cumsum([k.size for k in keys])]).astype(np.int64)
    total = int(koff[-1])
    mk = torch.full((max(total, 1),), -77, dtype=torch.int64, device=DEV)
    mp = torch.full((max(total, 1),), -77, dtype=torch.int64, device=DEV)
    cnt = torch.full((1,), 123, dtype=torch.int64, device=DEV)
    handles = (C.c_void_p * T_)(*[e.handle.value for e in evs])
    nd = None if n_dev is None else (C.c_void_p * T_)(*[None if n is None else n.data_ptr()
                                                        for n in n_dev])
    dr._lib.check(dr._lib.lib().dr_ev_missing_keys(
        handles, T_, flat.data_ptr() if total else None, (C.c_int64 * (T_ + 1))(*koff.tolist()),
        nd, mk.data_ptr(), mp.data_ptr(), cnt.data_ptr(),
        torch.cuda.current_stream().cuda_stream))
    m = int(cnt.item())
    got = sorted(zip(mp[:m].cpu().tolist(), mk[:m].cpu().tolist()))
    assert (mk[m:] == -77).all() and (mp[m:] == -77).all()      # nothing past the count
    return got, koff


@pytest.fixture(scope="module")
def filled(dr, uni):
    """Three EVs holding different parts of the universe (the last a Counter
    EV, filter_freq 3, whose keys were seen once), and for each the member
    keys by numpy: export() plus the keys key_meta() finds a row for."""
    rng = np.random.default_rng(3)
    evs = [make(dr, False), make(dr, False), make(dr, False, filter_freq=3)]
    members = []
    for i, ev in enumerate(evs):
        k = np.concatenate([rng.choice(uni.keys, 700, replace=False), uni.groups[0],
                            np.array([-1, 0], np.int64)[:2 - i]])
        ev.sparse_read(T(k))
        has = ev.key_meta(uni.keys)[2]
        exp = ev.export()[0].cpu().numpy()
        if i == 2:      # below filter_freq: in the map, not exported, and not missing
            assert exp.size == 0
            fr = ev.key_meta(uni.keys)[0]
            mem = uni.keys[fr >= 1]
            assert mem.size == np.unique(k).size
        else:
            mem = np.union1d(exp, uni.keys[has])
        members.append(mem)
    return evs, members


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049])
@pytest.mark.parametrize("tables", [1, 3])
def test_missing_keys_matches_numpy(dr, uni, filled, n, tables):
    evs, members = filled
    evs, members = evs[3 - tables:], members[3 - tables:]
    rng = np.random.default_rng([n, tables])
    never = np.arange(1 << 40, (1 << 40) + 500, dtype=np.int64)
    before = [(snap(e), e.rows_allocated()) for e in evs]
    keys = []
    for t in range(tables):
        nt = n if t == 0 else int(rng.integers(0, 300))
        pool = np.concatenate([members[t], never, uni.groups[0], uni.keys[:400]])
        k = rng.choice(pool, nt) if nt else np.zeros(0, np.int64)
        if nt > 8:
            k[:4] = k[4:8]                  # duplicates of residents and strangers alike
        keys.append(k.astype(np.int64))
    for cut in (False, True):
        n_dev, lim = None, [k.size for k in keys]
        if cut:
            lim = [int(k.size * 0.6) for k in keys]
            n_dev = [T(np.array([x], np.int64)) for x in lim]
            if tables > 1:      # a table without a device count beside those with one
                n_dev[-1], lim[-1] = None, keys[-1].size
        got, koff = missing(dr, evs, keys, n_dev)
        want = []
        for t, k in enumerate(keys):
            miss = ~np.isin(k[:lim[t]], members[t])
            want += [(int(koff[t]) + int(i), int(k[i])) for i in np.nonzero(miss)[0]]
        assert got == sorted(want)
    for e, (s, rows) in zip(evs, before):   # nothing in any table is written
        same(snap(e), s, "export after dr_ev_missing_keys")
        assert e.rows_allocated() == rows
    dr.status_check()


# ---------------------------------------------------------------------------
# 2. demote_to's victims are shrink_to's
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_demote_victims_are_shrink_to_victims(dr, uni, policy):
    ff = 2 if policy == "lfu" else 0
    a, b = make(dr, True, policy=policy, filter_freq=ff), make(dr, False, filter_freq=ff)
    opt = dr.AdagradOptimizer(L.LR)
    cols_a, cols_b = [[e, e.slot("Adagrad", opt.init_acc)] for e in (a, b)]
    b.track_removals()
    rng = np.random.default_rng(9)
    for step in range(6):
        keys = rng.choice(uni.keys, 350)
        if step == 5:
            keys = np.concatenate([keys[:100], rng.choice(uni.keys, 60, replace=False)])
        for ev in (a, b):
            if step < 5:
                train(dr, opt, ev, keys, step)
            else:       # seen, not trained: slot column untouched, Counter keys below filter_freq
                ev.sparse_read(T(keys))
    assert a.tier_count() == 0
    K = 500
    k0, v0, ve0, fr0 = snap(a)
    s0 = snap(cols_a[1])
    frq, ver, has = a.key_meta(uni.keys)
    live = uni.keys[has | (frq >= 1)] if ff else uni.keys[has]
    assert live.size == int(a.total_count()[0]) > K
    got = a.demote_to(K, policy, compact=True)
    assert got == b.shrink_to(K, policy) == live.size - K
    tk, tve, tfr, tcm, tv0, tv1 = tier_state(a)
    assert np.array_equal(tk, b.export_removed().cpu().numpy())
    assert a.tier_count() == got
    for ca, cb in zip(cols_a, cols_b):      # HBM's side of the merged export is the twin's
        ka = ca.export()[0].cpu().numpy()
        hbm = ~np.isin(ka, tk)
        same([x[hbm] if x.shape[:1] == ka.shape else x for x in snap(ca)],
             [x for x in snap(cb)], "HBM after demote_to against the twin after shrink_to")
    assert a.rows_allocated() == int(a.total_count()[0]) <= K
    assert not a.tracking_removals()
    # what the tier holds is what export() / key_meta said before the call
    i = np.searchsorted(uni.keys[np.argsort(uni.keys)], tk)
    order = np.argsort(uni.keys)
    assert np.array_equal(uni.keys[order][i], tk)
    assert np.array_equal(tve, ver[order][i])
    if ff:
        assert np.array_equal(tfr, frq[order][i])
    for col, (ek, ev_) in enumerate(((k0, v0), (s0[0], s0[1]))):
        touched = np.isin(tk, ek)
        assert np.array_equal(((tcm >> col) & 1).astype(bool) & (tcm & 1).astype(bool), touched)
        rows = (tv0, tv1)[col][touched].view(np.uint32)
        assert np.array_equal(rows, ev_[np.isin(ek, tk)])
    assert (~(tcm >> 1 & 1).astype(bool)).any()       # keys whose slot column was never touched
    dr.status_check()


def test_demote_keeps_the_removal_log(dr, uni):
    """dr_ev_demote_to on an EV that logs removals: the victims are not logged
    (a demoted key leaves HBM, not the model); dr_ev_shrink_to logs them."""
    ev = make(dr, False)
    ev.track_removals()
    ev.sparse_read(T(uni.keys[:900]))
    gone = ev.remove(T(uni.keys[:5]))
    assert gone == 5
    log0 = ev.export_removed().cpu().numpy()
    E = 895 - 700
    keys = torch.empty(E, dtype=torch.int64, device=DEV)
    m = C.c_int64(0)
    dr._lib.check(dr._lib.lib().dr_ev_demote_to(ev.handle, 700, 0, keys.data_ptr(), None, 0, None,
                                                None, None, E, C.byref(m),
                                                torch.cuda.current_stream().cuda_stream))
    assert m.value == E and int(ev.total_count()[0]) == 700
    assert np.array_equal(ev.export_removed().cpu().numpy(), log0)
    k = keys.cpu().numpy()
    assert (np.diff(k) > 0).all() and not np.isin(k, ev.export()[0].cpu().numpy()).any()
    assert ev.shrink_to(650) == 50
    assert ev.export_removed().numel() == 55
    dr.status_check()


# ---------------------------------------------------------------------------
# 3. promote is the exact inverse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float64"])
def test_promote_is_exact(dr, uni, dtype):
    a = make(dr, True, dtype=dtype, policy="lfu", filter_freq=3)
    opt = dr.GradientDescentOptimizer(L.LR)
    cols = [a, a.slot("acc", 0.25)]     # (fp32 rows beside a bf16 primary, float64 beside float64)
    rng = np.random.default_rng(4)
    trained = rng.choice(uni.keys, 500, replace=False)
    for step in range(4):       # four sightings: admitted, rows written
        train(dr, opt, a, trained, step, dtype=dtype)
    cols[1].insert(T(trained[:300]), T(rng.integers(-8, 9, (300, DIM)) * 0.5))
    seen = rng.choice(uni.keys[~np.isin(uni.keys, trained)], 300, replace=False)
    a.insert(T(seen[:150]), T(np.full((150, DIM), 2.5)), T(np.arange(150)), T(np.full(150, 7)))
    a.sparse_read(T(seen[150:]))    # once: in the map below filter_freq, no column touched
    before = [snap(c) for c in cols]
    meta = a.key_meta(uni.keys)
    n = int(a.total_count()[0])
    assert n == 800
    # keys whose slot column was never touched, Counter keys below filter_freq: both present
    assert before[1][0].size == 300 and before[0][0].size == 650
    assert (meta[0][np.isin(uni.keys, seen[150:])] == 1).all()
    assert a.demote_to(0) == n and int(a.total_count()[0]) == 0 and a.rows_allocated() == 0
    assert a.tier_count() == n
    for c, s in zip(cols, before):  # export() merges the tiers
        same(snap(c), s, "merged export with everything demoted")
    assert not a.key_meta(uni.keys)[2].any()
    assert a.promote(T(uni.keys)) == n and a.tier_count() == 0
    assert int(a.total_count()[0]) == n
    for c, s in zip(cols, before):
        same(snap(c), s, "export after demote_to(0) and promote(all)")
    for x, y in zip(a.key_meta(uni.keys), meta):
        assert np.array_equal(x, y)
    # a column that was untouched is initialised by its next first touch, as for a new key
    k = before[0][0][~np.isin(before[0][0], before[1][0])][:20]
    assert k.size == 20
    assert (cols[1].sparse_read(T(k)) == cols[1].default_value).all()
    dr.status_check()


# ---------------------------------------------------------------------------
# 4. the main test: a tiered walk equals its twin
# ---------------------------------------------------------------------------
WALKS = [(21, "float32", "sgd", "lru", 0), (22, "float32", "adagrad", "lru", 0),
         (23, "bfloat16", "sgd", "lru", 0), (24, "float64", "sgd", "lru", 0),
         (25, "float32", "adagrad", "lfu", 3)]


@pytest.mark.parametrize("seed,dtype,optname,policy,ff", WALKS,
                         ids=["%s-%s-%s" % w[1:4] for w in WALKS])
def test_tiered_walk_equals_twin(dr, seed, dtype, optname, policy, ff):
    uni = L.universe(seed)
    a = make(dr, True, dtype=dtype, policy=policy, filter_freq=ff)
    b = make(dr, False, dtype=dtype, filter_freq=ff)
    if optname == "adagrad":
        opt = dr.AdagradOptimizer(L.LR)
        cols_a, cols_b = [[e, e.slot("Adagrad", opt.init_acc)] for e in (a, b)]
    else:
        opt = dr.GradientDescentOptimizer(L.LR)
        cols_a, cols_b = [a], [b]
    promoted, first_demotion, steps_promoting = 0, None, 0
    rng = np.random.default_rng([seed, 9])
    both = []
    for step, keys in enumerate(W.batches(seed)):
        t0 = a.tier_count()
        oa = train(dr, opt, a, keys, step, seed, dtype)
        p = t0 - a.tier_count()
        ob = train(dr, opt, b, keys, step, seed, dtype)
        assert np.array_equal(oa, ob), "step %d: the lookup's rows differ from the twin's" % step
        promoted += p
        steps_promoting += bool(p) and first_demotion is not None
        if step in (W.INSERT_AT, W.REMOVE_AT):     # an insert / a remove over both tiers
            in_hbm = a.key_meta(uni.keys)[2]
            tk = tier_state(a)[0]       # (with a Counter filter mostly keys below filter_freq)
            rest = ~in_hbm & ~np.isin(uni.keys, tk)
            k = np.concatenate([rng.choice(uni.keys[in_hbm], 60, replace=False),
                                rng.choice(tk, 60, replace=False),
                                rng.choice(uni.keys[rest], 30, replace=False)])
            both.append(step)
            if step == W.INSERT_AT:
                for ev in (a, b):
                    ev.insert(T(k), T(np.full((k.size, DIM), -1.5)), T(np.full(k.size, step)),
                              T(np.full(k.size, 5)))
            else:
                t0 = a.tier_count()
                ra, rb = a.remove(T(k)), b.remove(T(k))
                assert ra == rb >= 120 and t0 - a.tier_count() == 60, (ra, rb)
        if (step + 1) % W.DEMOTE_EVERY == 0:
            if a.demote_to(W.BUDGET) and first_demotion is None:
                first_demotion = step
            assert int(a.total_count()[0]) <= W.BUDGET
        if (step + 1) % W.SHRINK_EVERY == 0:
            assert a.shrink(step) == b.shrink(step)
    assert both == [W.INSERT_AT, W.REMOVE_AT]
    for ca, cb in zip(cols_a, cols_b):
        same(snap(ca), snap(cb), "export() of %s against the twin" % ca.name)
    assert a.tier_count() > 0
    # the walk proves something only if keys came back from the tier, often
    after = W.STEPS - 1 - first_demotion
    assert promoted >= 200 and steps_promoting * 2 >= after, (promoted, steps_promoting, after)
    dr.status_check()


def test_slot_created_after_a_demotion(dr, uni):
    """An optimizer slot that appears once the tier already holds keys: the
    host store moves to a wider one, the new column untouched for every key it
    held, and the walk goes on equal to the twin's."""
    a, b = make(dr, True, max_keys=300), make(dr, False)
    sgd, ada = dr.GradientDescentOptimizer(L.LR), dr.AdagradOptimizer(L.LR)
    rng = np.random.default_rng(17)
    for step in range(4):
        keys = rng.choice(uni.keys[:1000], 300)
        for ev in (a, b):
            train(dr, sgd, ev, keys, step)
    assert a.demote_to() > 0 and a._tier_ncols == 1
    t0 = tier_state(a)
    slots = [e.slot("Adagrad", ada.init_acc) for e in (a, b)]
    promoted = 0
    for step in range(4, 10):
        keys = rng.choice(uni.keys[:1000], 300)
        n0 = a.tier_count()
        oa = train(dr, ada, a, keys, step)
        promoted += n0 - a.tier_count()
        assert np.array_equal(oa, train(dr, ada, b, keys, step))
        if step == 4:       # the first demotion with two columns widened the store
            a.demote_to()
            assert a._tier_ncols == 2
            k, ve, fr, cm = tier_state(a)[:4]
            old = np.isin(k, t0[0]) & ~np.isin(k, np.unique(keys))
            assert old.any() and ((cm[old] >> 1) & 1 == 0).all()
        elif step % 2 == 0:
            a.demote_to()
    assert promoted > 100
    for ca, cb in zip([a, slots[0]], [b, slots[1]]):
        same(snap(ca), snap(cb), "export() of %s against the twin" % ca.name)
    dr.status_check()


# ---------------------------------------------------------------------------
# 5. grouped lookups
# ---------------------------------------------------------------------------
def test_tiered_grouped_paths_equal_twin(dr, uni):
    from deeprec_amd.kv_variable_ops import PendingRowSlices
    rng = np.random.default_rng(6)
    As = [make(dr, True, max_keys=300) for _ in range(3)]
    Bs = [make(dr, False) for _ in range(3)]
    opt = dr.GradientDescentOptimizer(L.LR)
    B = 256
    ind1 = T(np.stack([np.arange(B), np.zeros(B, np.int64)], 1))
    promoted = 0
    for step in range(10):
        ids = [rng.choice(uni.keys[:900], B) for _ in range(3)]
        g = rng.integers(-2, 3, (B, 3 * DIM)).astype(np.float32)
        outs = []
        for evs in (As, Bs):
            t0 = sum(e.tier_count() for e in evs)
            sps = [dr.SparseTensor(ind1, T(k), (B, 1)) for k in ids]
            out = dr.embedding_lookup_sparse_multi(evs, sps, combiner="sum")
            promoted += t0 - sum(e.tier_count() for e in evs)
            out.backward(T(g))
            # the fused path: the one-hot probe + copy kernel recorded the rows, the
            # backward is still unformed and SGD runs fused with it
            pend = [e.pending_grads[-1] for e in evs]
            assert all(isinstance(p, PendingRowSlices) and p.fusable() for p in pend)
            opt.apply_gradients(evs, global_step=step)
            assert all(p._pending.applied for p in pend)
            outs.append(bits(out.detach()))
        assert np.array_equal(*outs), "step %d: one-hot grouped lookup" % step
        if step % 3 == 2:   # the forward-only fused one-hot lookup (no gradient recorded)
            ids2 = [rng.choice(uni.keys[:900], B) for _ in range(3)]
            outs = []
            for evs in (As, Bs):
                t0 = sum(e.tier_count() for e in evs)
                with torch.no_grad():
                    outs.append(bits(dr.embedding_lookup_sparse_multi(
                        evs, [dr.SparseTensor(ind1, T(k), (B, 1)) for k in ids2],
                        combiner="sum")))
                promoted += t0 - sum(e.tier_count() for e in evs)
            assert np.array_equal(*outs), "step %d: forward-only one-hot lookup" % step
        # a multi-hot bag lookup with combiner="mean" on the first EV
        nnz = 600
        rows = np.sort(rng.integers(0, B, nnz))
        cols = np.zeros(nnz, np.int64)
        for i in range(1, nnz):
            cols[i] = cols[i - 1] + 1 if rows[i] == rows[i - 1] else 0
        mk = rng.choice(uni.keys[:900], nnz)
        gm = rng.integers(-2, 3, (B, DIM)).astype(np.float32)
        outs = []
        for ev in (As[0], Bs[0]):
            t0 = ev.tier_count()
            sp = dr.SparseTensor(T(np.stack([rows, cols], 1)), T(mk), (B, int(cols.max()) + 1))
            out = dr.embedding_lookup_sparse(ev, sp, combiner="mean")
            promoted += t0 - ev.tier_count()
            out.backward(T(gm))
            opt.apply_gradients([ev], global_step=step)
            outs.append(bits(out.detach()))
        assert np.array_equal(*outs), "step %d: multi-hot mean lookup" % step
        if step % 2 == 1:
            for e in As:
                e.demote_to()
                assert int(e.total_count()[0]) <= 300
    assert promoted >= 200, promoted
    for ea, eb in zip(As, Bs):
        same(snap(ea), snap(eb), "export() after grouped lookups")
    dr.status_check()


def test_tiered_per_feature_and_chunked_promotion(dr, uni, monkeypatch):
    """Two grouped routes the main test does not take: features of different
    dims are resolved one by one (_prepare) after ONE grouped promotion, and
    more than MAX_GROUP tiered EVs are promoted in chunks."""
    import deeprec_amd.kv_variable_ops as kv
    rng = np.random.default_rng(19)
    As = [make(dr, True, max_keys=200, dim=d) for d in (8, 16)]
    Bs = [make(dr, False, dim=d) for d in (8, 16)]
    opt = dr.GradientDescentOptimizer(L.LR)
    B = 200
    ind1 = T(np.stack([np.arange(B), np.zeros(B, np.int64)], 1))
    calls = []
    real = kv._tier_misses
    monkeypatch.setattr(kv, "_tier_misses", lambda items: calls.append(len(items)) or real(items))
    promoted = 0
    for step in range(6):
        ids = [rng.choice(uni.keys[:700], B) for _ in range(2)]
        g = rng.integers(-2, 3, (B, 24)).astype(np.float32)
        outs = []
        for evs in (As, Bs):
            del calls[:]
            t0 = sum(e.tier_count() for e in evs)
            n_t = sum(1 for e in evs if e.tier_count())
            out = dr.embedding_lookup_sparse_multi(
                evs, [dr.SparseTensor(ind1, T(k), (B, 1)) for k in ids], combiner="sum")
            promoted += t0 - sum(e.tier_count() for e in evs)
            if evs is As and t0:    # one missing-keys launch for the group, none per feature
                assert calls == [n_t], calls
            out.backward(T(g))
            opt.apply_gradients(evs, global_step=step)
            outs.append(bits(out.detach()))
        assert np.array_equal(*outs), "step %d" % step
        for e in As:
            e.demote_to()
    assert promoted > 100
    for ea, eb in zip(As, Bs):
        same(snap(ea), snap(eb), "export() after per-feature lookups")
    monkeypatch.undo()
    # 33 tiered EVs in one promote_grouped: two chunks
    n_ev = dr._lib.MAX_GROUP + 1
    evs = [make(dr, True, max_keys=10) for _ in range(n_ev)]
    keys = [T(uni.keys[40 * (i % 50):40 * (i % 50) + 40]) for i in range(n_ev)]
    for e, k in zip(evs, keys):
        e.sparse_read(k)
    before = [snap(e) for e in evs]
    assert all(e.demote_to() == 30 for e in evs)
    assert kv.promote_grouped(evs, keys) == 30 * n_ev
    assert all(e.tier_count() == 0 and int(e.total_count()[0]) == 40 for e in evs)
    for e, s in zip(evs, before):
        same(snap(e), s, "export() after a chunked promotion")
    dr.status_check()


# ---------------------------------------------------------------------------
# 6. read-only lookups
# ---------------------------------------------------------------------------
def test_tiered_read_only(dr, uni):
    a, b = make(dr, True, filter_freq=2), make(dr, False, filter_freq=2)
    opt = dr.GradientDescentOptimizer(L.LR)
    rng = np.random.default_rng(8)
    for step in range(5):
        keys = rng.choice(uni.keys[:1200], 380)
        for ev in (a, b):
            train(dr, opt, ev, keys, step)
    once = uni.keys[1200:1260]
    for ev in (a, b):
        ev.sparse_read(T(once))     # below filter_freq: read-only serves the default
    assert a.demote_to(400) > 0
    tk = tier_state(a)[0]
    never = np.arange(1 << 41, (1 << 41) + 40, dtype=np.int64)
    q = np.concatenate([tk[:200], tk[:50], once, never, a.export()[0].cpu().numpy()[:100]])
    q = rng.permutation(q)
    hbm0, tier0 = snap(a), tier_state(a)
    ra = bits(a.sparse_read(T(q), read_only=True))
    assert np.array_equal(ra, bits(b.sparse_read(T(q), read_only=True)))
    dflt = bits(a.default_value.reshape(1, DIM))
    assert (ra[np.isin(q, never)] == dflt).all() and (ra[np.isin(q, once)] == dflt).all()
    assert (ra[np.isin(q, tk)] != dflt).any()
    with dr.read_only_lookups():
        rl = dr.embedding_lookup(a, T(q.reshape(-1, 2)))
        assert np.array_equal(bits(rl).reshape(-1, DIM), ra)
        ev3 = T(np.full((q.size, DIM), 3.0, np.float32))
        assert np.array_equal(bits(dr.embedding_lookup(a, T(q), ev_init_value=ev3)),
                              bits(dr.embedding_lookup(b, T(q), ev_init_value=ev3)))
        # pooled read-only lookups read HBM's pool by index: tier-resident ids are refused
        Bn = 64
        ind = T(np.stack([np.arange(Bn), np.zeros(Bn, np.int64)], 1))
        with pytest.raises(dr.InvalidArgumentError, match=r"promote\(keys\) first"):
            dr.embedding_lookup_sparse(a, dr.SparseTensor(ind, T(tk[:Bn]), (Bn, 1)),
                                       combiner="sum")
        res = a.export()[0].cpu().numpy()
        res = res[~np.isin(res, tk)][:Bn]
        sp = dr.SparseTensor(ind, T(res), (Bn, 1))
        assert np.array_equal(bits(dr.embedding_lookup_sparse(a, sp, combiner="sum")),
                              bits(dr.embedding_lookup_sparse(b, sp, combiner="sum")))
    same(snap(a), hbm0, "the merged export after read-only lookups")
    same(tier_state(a), tier0, "the host tier after read-only lookups")
    dr.status_check()


# ---------------------------------------------------------------------------
# 7. checkpoints
# ---------------------------------------------------------------------------
def test_tiered_checkpoint_bytes_equal_twin(dr, uni, tmp_path):
    from deeprec_amd import checkpoint as ck
    a, b = make(dr, True, max_keys=500), make(dr, False)
    opt = dr.AdagradOptimizer(L.LR)
    rng = np.random.default_rng(12)
    va, vb = [{"emb": e, "emb/Adagrad": e.slot("Adagrad", opt.init_acc)} for e in (a, b)]
    for step in range(30):
        keys = rng.choice(uni.keys[:1500], 300)
        for ev in (a, b):
            train(dr, opt, ev, keys, step)
        if step == 14:
            a.demote_to()
    pa = ck.save(str(tmp_path / "tiered"), va, global_step=29, compact=True)
    pb = ck.save(str(tmp_path / "twin"), vb, global_step=29, compact=True)
    assert int(a.total_count()[0]) <= 500 and a.tier_count() > 0
    assert a.rows_allocated() == int(a.total_count()[0])
    for ext in (".index", ".data-00000-of-00001"):
        assert filecmp.cmp(pa + ext, pb + ext, shallow=False), ext
    c, d = make(dr, True, max_keys=500), make(dr, False)
    vc, vd = [{"emb": e, "emb/Adagrad": e.slot("Adagrad", opt.init_acc)} for e in (c, d)]
    ck.restore(pa, vc)
    ck.restore(pb, vd)
    assert int(c.total_count()[0]) <= 500 and c.tier_count() > 0
    for name in vc:
        same(snap(vc[name]), snap(vd[name]), "restored %s" % name)
    dr.status_check()


# ---------------------------------------------------------------------------
# 8. what is refused
# ---------------------------------------------------------------------------
def test_tiered_refusals(dr, uni):
    HD = dr.StorageOption(dr.StorageType.HBM_DRAM)
    bud = dr.KeyBudgetEvict(100, "lru", steps_to_live=5)

    def ctor(**kw):
        o = dict(evict_option=bud, storage_option=HD)
        o.update(kw.pop("opt", {}))
        return dr.EmbeddingVariable("tier_refused", DIM, 0.5, device=DEV,
                                    ev_option=dr.EmbeddingVariableOption(**o), **kw)

    for kw in (dict(opt=dict(evict_option=None)),
               dict(opt=dict(evict_option=dr.GlobalStepEvict(5))),
               dict(opt=dict(filter_option=dr.CBFFilter(2, max_element_size=1000,
                                                        false_positive_probability=0.01))),
               dict(key_dtype=torch.int32), dict(l2_weight_threshold=0.1)):
        with pytest.raises(dr.InvalidArgumentError, match="HBM_DRAM needs"):
            ctor(**kw)
    a = make(dr, True, max_keys=200)
    assert a.tiered and not make(dr, False).tiered
    for call in (a.track_updates, a.track_removals):
        with pytest.raises(dr.InvalidArgumentError, match="host-DRAM tier"):
            call()
    with pytest.raises(dr.InvalidArgumentError, match="HBM_DRAM"):
        make(dr, False).demote_to(10)
    keys = uni.keys[:600]
    a.sparse_read(T(keys))
    a.pending_grads.append(dr.IndexedSlices(T(np.zeros((4, DIM), np.float32)), T(keys[:4])))
    with pytest.raises(dr.InvalidArgumentError, match="pending gradient"):
        a.demote_to()
    a.pending_grads.clear()
    # a slot handle, and a capacity below the victim count: table and tier unchanged
    slot = a.slot("Adagrad", 0.1)
    lib, st = dr._lib.lib(), torch.cuda.current_stream().cuda_stream
    s0, m = snap(a), C.c_int64(-5)
    buf = torch.empty(600, dtype=torch.int64, device=DEV)
    assert lib.dr_ev_demote_to(slot.handle, 200, 0, buf.data_ptr(), None, 0, None, None, None, 600,
                               C.byref(m), st) == dr._lib.INVALID_ARGUMENT
    assert lib.dr_ev_demote_to(a.handle, 200, 0, buf.data_ptr(), None, 0, None, None, None, 399,
                               C.byref(m), st) == dr._lib.INVALID_ARGUMENT
    assert lib.dr_ev_demote_to(a.handle, 200, 0, None, None, 0, None, None, None, 0,
                               C.byref(m), st) == 0 and m.value == 400     # the query
    assert int(a.total_count()[0]) == 600 and a.tier_count() == 0
    same(snap(a), s0, "after refused demotions")
    assert a.demote_to() == 400
    # incremental checkpoints and the sharded engines: refused before anything changes
    from deeprec_amd import checkpoint as ck
    from deeprec_amd.sharded import HipLocal
    tier0 = tier_state(a)
    rows0 = a.rows_allocated()
    for call in (lambda: ck.save_incremental("/nonexistent/never_written", {"emb": a}, 3),
                 lambda: ck.save_incremental("/nonexistent/never_written", {"emb/s": slot}),
                 lambda: ck.restore_incremental("/nonexistent/never_read", {"emb": a})):
        with pytest.raises(dr.InvalidArgumentError, match="host-DRAM tier"):
            call()
    with pytest.raises(dr.InvalidArgumentError, match="does not promote"):
        HipLocal([a], a.device)
    assert int(a.total_count()[0]) == 200 and a.rows_allocated() == rows0
    same(tier_state(a), tier0, "the host tier after refused incremental checkpoints")
    same(snap(a), s0, "the merged export after refused incremental checkpoints")
    # stream capture with keys in the tier
    g = torch.cuda.CUDAGraph()
    k, x, err, err_ro = T(keys[:64]), torch.zeros(8, device=DEV), None, None
    with torch.cuda.graph(g):
        x += 1
        try:
            a.sparse_read(k)
        except dr.InvalidArgumentError as e:
            err = e
        try:
            a.sparse_read(k, read_only=True)
        except dr.InvalidArgumentError as e:
            err_ro = e
        rc = lib.dr_ev_demote_to(a.handle, 100, 0, buf.data_ptr(), None, 0, None, None, None, 600,
                                 C.byref(m), torch.cuda.current_stream().cuda_stream)
    assert err is not None and "cannot be captured" in str(err)
    assert "read-only" in str(err_ro) and "cannot be captured" in str(err_ro)
    assert rc == dr._lib.INVALID_ARGUMENT
    g.replay()
    torch.cuda.synchronize()
    assert a.tier_count() == 400 and int(a.total_count()[0]) == 200
    same(snap(a), s0, "after a refused capture")
    dr.status_check()
