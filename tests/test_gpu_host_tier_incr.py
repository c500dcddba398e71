"""GPU: incremental checkpoints of a tiered (HBM + host-DRAM) EmbeddingVariable
(StorageOption(StorageType.HBM_DRAM, incremental=True)).

Section 16's transparency contract, extended to deltas: a tiered trainer that
tracks updates, logs removals and writes incremental checkpoints is observably
equal to an untiered, unbudgeted twin that saw the same calls -- bit-equal
export_updated() of the primary and the slot, equal export_removed(),
byte-equal delta bundles.  Everything is compared bit for bit; no tolerance
appears anywhere.

capacity=1 (1 024 rows, so the tables grow while the tier holds marked keys),
dim 8, about 1 500 keys of ev_lifecycle.universe (the four special keys,
clustered groups), HBM budgets of 200-400 keys; values and gradients are
multiples of 0.5.
"""
import ctypes as C
import filecmp

import numpy as np
import pytest
import torch

import ev_lifecycle as L
import host_tier_incr_walk as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIM = W.DIM
UPDATED = 1 << 16
TORCH_DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float64": torch.float64}


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    return deeprec_amd


@pytest.fixture(scope="module")
def uni():
    return W.universe(7)[0]


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def bits(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy()
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def tup(x):
    k, v, ve, fr = x
    return k.cpu().numpy(), bits(v), ve.cpu().numpy(), fr.cpu().numpy()


def same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, i, x.shape, y.shape)
        assert np.array_equal(x, y), "%s: field %d differs, first at %s" % (
            what, i, np.argwhere(x != y)[0].tolist())


_N = [0]


def make(dr, tiered, incremental=True, dtype="float32", policy="lru", filter_freq=0, max_keys=300,
         stl=W.STEPS_TO_LIVE):
    """An opted-in tiered EV, or its twin: untiered and unbudgeted, otherwise the same."""
    _N[0] += 1
    evict = dr.KeyBudgetEvict(max_keys, policy, steps_to_live=stl) if tiered \
        else dr.GlobalStepEvict(stl)
    so = dr.StorageOption(dr.StorageType.HBM_DRAM, incremental=True) if incremental \
        else dr.StorageOption(dr.StorageType.HBM_DRAM)
    opt = dr.EmbeddingVariableOption(
        evict_option=evict,
        filter_option=dr.CounterFilter(filter_freq) if filter_freq else None,
        storage_option=so if tiered else None)
    return dr.EmbeddingVariable("tincr_%d_%s" % (_N[0], "a" if tiered else "b"), DIM, L.DEFAULT,
                                ev_option=opt, device=DEV, value_dtype=TORCH_DT[dtype], capacity=1)


def grads(seed, step, n):
    return np.random.default_rng([seed, 8, step]).integers(-2, 3, (n, DIM)).astype(np.float32)


def train(dr, opt, ev, keys, gs, seed=0):
    """One step: the lookup of `keys` (duplicates and all), then the optimizer
    on the distinct keys with global_step = gs."""
    ev.sparse_read(T(keys))
    u = np.unique(keys)
    ev.pending_grads.append(dr.IndexedSlices(T(grads(seed, gs, u.size)), T(u)))
    opt.apply_gradients([ev], global_step=gs)


def train_rows(dr, opt, ev, keys, gs, seed=0):
    """The same step through a forward that records the rows it resolved
    (a one-hot embedding_lookup_sparse and its backward): with
    track_updates(by_row=True) the apply marks by row, without a probe."""
    B = keys.size
    ind = T(np.stack([np.arange(B), np.zeros(B, np.int64)], 1))
    out = dr.embedding_lookup_sparse(ev, dr.SparseTensor(ind, T(keys), (B, 1)), combiner="sum")
    out.backward(T(grads(seed, gs, B)))
    opt.apply_gradients([ev], global_step=gs)
    assert not ev.pending_grads


# ---------------------------------------------------------------------------
# 1. C level: the bit leaves with the victim and comes back with the key
# ---------------------------------------------------------------------------
def c_demote(dr, ev, cols, max_keys, policy=0):
    lib, st = dr._lib.lib(), torch.cuda.current_stream().cuda_stream
    m = C.c_int64(0)
    dr._lib.check(lib.dr_ev_demote_to(ev.handle, max_keys, policy, None, None, 0, None, None, None,
                                      0, C.byref(m), st))
    E = m.value
    keys = torch.empty(E, dtype=torch.int64, device=DEV)
    vers, frqs = torch.empty_like(keys), torch.empty_like(keys)
    cm = torch.empty(E, dtype=torch.int32, device=DEV)
    vals = [torch.empty((E, c.dim), dtype=c.value_dtype, device=DEV) for c in cols]
    vptr = (C.c_void_p * len(cols))(*[v.data_ptr() for v in vals])
    dr._lib.check(lib.dr_ev_demote_to(ev.handle, max_keys, policy, keys.data_ptr(), vptr, len(cols),
                                      vers.data_ptr(), frqs.data_ptr(), cm.data_ptr(), E,
                                      C.byref(m), st))
    assert m.value == E
    return keys, vals, vers, frqs, cm


def c_promote(dr, ev, keys, vals, vers, frqs, cm):
    vptr = (C.c_void_p * len(vals))(*[v.data_ptr() for v in vals])
    dr._lib.check(dr._lib.lib().dr_ev_promote(
        ev.handle, keys.data_ptr(), keys.numel(), vptr, len(vals), vers.data_ptr(), frqs.data_ptr(),
        cm.data_ptr(), torch.cuda.current_stream().cuda_stream))


def filled(dr, uni, dtype, track):
    """900 keys looked up (the primary touched), the slot column written for
    500 of them, 400 marked through the public route (absent keys among them)."""
    rng = np.random.default_rng(3)
    ev = make(dr, False, dtype=dtype)
    slot = ev.slot("acc", 0.25)
    keys = np.concatenate([uni[:4], rng.choice(uni[4:], 896, replace=False)])
    ev.sparse_read(T(keys))
    slot.insert(T(keys[:500]), T(rng.integers(-8, 9, (500, DIM)) * 0.5))
    # versions spread over 0..8 so that the LRU victims are not simply the smallest keys
    ev.upsert(T(keys), T(rng.integers(-8, 9, (900, DIM)) * 0.5), T(rng.integers(0, 9, 900)))
    marked = np.concatenate([keys[:2], rng.choice(keys, 398, replace=False),
                             np.arange(1 << 40, (1 << 40) + 20)])
    if track:
        ev.track_updates()
        ev.mark_updated(T(marked))
    return ev, slot, keys, np.unique(marked)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float64"])
def test_update_bit_round_trip(dr, uni, dtype):
    ev, slot, keys, marked = filled(dr, uni, dtype, True)
    before = [tup(c.export_updated()) for c in (ev, slot)]
    full = [tup(c.export()) for c in (ev, slot)]
    assert np.array_equal(before[0][0], np.intersect1d(marked, keys))
    assert 0 < before[1][0].size < before[0][0].size      # marked keys without a slot row
    assert ev.rows_allocated() == 900
    k, vals, vers, frqs, cm = c_demote(dr, ev, [ev, slot], 300)
    hk, hcm = k.cpu().numpy(), cm.cpu().numpy().view(np.uint32)
    assert hk.size == 600 and (np.diff(hk) > 0).all()
    # bit 16 exactly for the victims that were in export_updated() just before
    assert np.array_equal((hcm & UPDATED) != 0, np.isin(hk, before[0][0]))
    flagged = int(((hcm & UPDATED) != 0).sum())
    assert 100 < flagged < 400 and ((hcm >> 17) == 0).all() and ((hcm & 1) == 1).all()
    left = tup(ev.export_updated())
    assert np.array_equal(left[0], before[0][0][~np.isin(before[0][0], hk)])
    # the inverse, on new rows: 900 + 600 rows force a growth past 1 024 with marks held
    c_promote(dr, ev, k, vals, vers, frqs, cm)
    assert ev.rows_allocated() == 1500
    for c, b, f in zip((ev, slot), before, full):
        same(tup(c.export_updated()), b, "export_updated of %s after the round trip" % c.name)
        same(tup(c.export()), f, "export of %s after the round trip" % c.name)
    assert ev.updated_count() >= before[0][0].size
    # a key already in the map, and a repeated key, are left as they are
    ev.clear_updated()
    c_promote(dr, ev, k, vals, vers, frqs, cm)
    assert ev.export_updated()[0].numel() == 0 and ev.rows_allocated() == 1500
    dr.status_check()


def test_update_bit_is_ignored_without_tracking(dr, uni):
    ev, slot, keys, _ = filled(dr, uni, "float32", False)
    full = [tup(c.export()) for c in (ev, slot)]
    k, vals, vers, frqs, cm = c_demote(dr, ev, [ev, slot], 300)
    hcm = cm.cpu().numpy().view(np.uint32)
    assert (hcm >> 16 == 0).all()                           # the parent's output: 16 bits
    c_promote(dr, ev, k, vals, vers, frqs, cm | UPDATED)    # bit 16 set: no error, no effect
    assert not ev.tracking_updates()
    for c, f in zip((ev, slot), full):
        same(tup(c.export()), f, "export of %s" % c.name)
    ev.track_updates()                                      # and nothing stale appears later
    assert ev.export_updated()[0].numel() == 0 and ev.updated_count() == 0
    dr.status_check()


def test_log_removed_appends_and_grows(dr, uni):
    lib, st = dr._lib.lib(), torch.cuda.current_stream().cuda_stream
    ev = make(dr, False)
    slot = ev.slot("acc", 0.25)
    a = T(np.concatenate([uni[:700], uni[:3]]))
    assert lib.dr_ev_log_removed(ev.handle, a.data_ptr(), a.numel(), st) == 0   # not logging
    assert not ev.tracking_removals()
    ev.track_removals()
    assert ev.removed_count() == 0
    assert lib.dr_ev_log_removed(ev.handle, a.data_ptr(), a.numel(), st) == 0
    assert lib.dr_ev_log_removed(ev.handle, None, 0, st) == 0
    assert ev.removed_count() == 703
    assert np.array_equal(ev.export_removed().cpu().numpy(), np.sort(uni[:700]))
    b = T(uni[600:1300])                                    # past the log's first 1 024 entries
    assert lib.dr_ev_log_removed(ev.handle, b.data_ptr(), b.numel(), st) == 0
    assert ev.removed_count() == 1403
    assert np.array_equal(ev.export_removed().cpu().numpy(), np.sort(uni[:1300]))
    ev.sparse_read(T(uni[:50]))                             # and remove() appends behind them
    assert ev.remove(T(np.arange(1 << 41, (1 << 41) + 5))) == 0
    assert ev.remove(T(uni[:10])) == 10
    assert ev.removed_count() == 1413
    assert np.array_equal(ev.export_removed().cpu().numpy(), np.sort(uni[:1300]))
    assert lib.dr_ev_log_removed(slot.handle, a.data_ptr(), 1, st) == dr._lib.INVALID_ARGUMENT
    assert lib.dr_ev_log_removed(ev.handle, None, 1, st) == dr._lib.INVALID_ARGUMENT
    ev.clear_removed()
    assert ev.export_removed().numel() == 0
    dr.status_check()


# ---------------------------------------------------------------------------
# 2. the twin walk
# ---------------------------------------------------------------------------
class Pair(object):
    """The opted-in tiered EV `a` and its twin `b` under one operation list."""

    def __init__(self, dr, case):
        self.dr, self.case = dr, case
        self.a = make(dr, True, policy=case.policy, filter_freq=case.filter_freq)
        self.b = make(dr, False, filter_freq=case.filter_freq)
        if case.opt == "adagrad":
            self.opt = dr.AdagradOptimizer(L.LR)
            self.cols = [[e, e.slot("Adagrad", self.opt.init_acc)] for e in (self.a, self.b)]
        else:
            self.opt = dr.GradientDescentOptimizer(L.LR)
            self.cols = [[e] for e in (self.a, self.b)]
        for e in (self.a, self.b):
            e.track_updates(by_row=case.by_row)
            e.track_removals()
        self.tracking = True

    def apply(self, op):
        a, b, name = self.a, self.b, op["op"]
        if name == "train":
            step = train_rows if self.case.by_row else train
            for e in (a, b):
                step(self.dr, self.opt, e, op["keys"], op["gs"], self.case.seed)
        elif name == "lookup":
            ra, rb = (bits(e.sparse_read(T(op["keys"]))) for e in (a, b))
            assert np.array_equal(ra, rb), "the lookup's rows differ from the twin's"
        elif name == "mark":
            for e in (a, b):
                e.mark_updated(T(op["keys"]))
        elif name == "demote":
            return a.demote_to(op["n"], self.case.policy, compact=op["compact"])
        elif name == "remove":
            ra, rb = a.remove(T(op["keys"])), b.remove(T(op["keys"]))
            assert ra == rb, ("remove", ra, rb)
            return ra
        elif name == "shrink":
            ra, rb = a.shrink(op["gs"]), b.shrink(op["gs"])
            assert ra == rb, ("shrink", ra, rb)
            return ra
        elif name == "clear":
            for e in (a, b):
                e.clear_updated()
        elif name in ("track_off", "track_on"):
            self.tracking = name == "track_on"
            for e in (a, b):
                e.track_updates(self.tracking, by_row=self.case.by_row)
        else:
            raise AssertionError("unknown operation %r" % name)
        return None

    def observe(self):
        """The tiered EV's state in the model's shapes, after checking it
        against the twin's field by field."""
        ca, cb = self.cols
        ex = [tup(c.export()) for c in ca]
        for c, x, d in zip(ca, ex, cb):
            same(x, tup(d.export()), "export() of %s against the twin" % c.name)
        rem = self.a.export_removed().cpu().numpy()
        assert np.array_equal(rem, self.b.export_removed().cpu().numpy()), \
            "export_removed() differs from the twin's"
        o = {"keys": ex[0][0], "versions": ex[0][2], "removed": rem,
             "slot_keys": ex[-1][0] if len(ca) > 1 else np.zeros(0, np.int64),
             "hbm_count": int(self.a.total_count()[0]), "tier_count": self.a.tier_count(),
             "rows": self.a.rows_allocated()}
        if self.tracking:
            up = [tup(c.export_updated()) for c in ca]
            for c, x, d in zip(ca, up, cb):
                same(x, tup(d.export_updated()), "export_updated() of %s against the twin" % c.name)
                assert c.updated_count() >= x[0].size
            o["updated"] = up[0][0]
            o["slot_updated"] = up[-1][0] if len(ca) > 1 else np.zeros(0, np.int64)
        return o


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_tiered_incremental_walk(dr, case):
    ops = W.generate(case)
    m, pair = W.Model(case), Pair(dr, case)
    for i, op in enumerate(ops):
        try:
            want = m.apply(op)
            got = pair.apply(op)
            if want is not None:
                assert got == want, "%s returned %r, the model has %r" % (op["op"], got, want)
            L.compare(pair.observe(), m.observe(), "the tiered EV")
        except AssertionError as e:
            raise AssertionError("%s\n%s" % (W.replay_info(case, ops, i), e)) from e
    assert pair.a.tier_count() > 0
    dr.status_check()


# ---------------------------------------------------------------------------
# 3. deltas: byte-equal bundles
# ---------------------------------------------------------------------------
def trainer_pair(dr, max_keys=300):
    a, b = make(dr, True, max_keys=max_keys), make(dr, False)
    opt = dr.AdagradOptimizer(L.LR)
    va, vb = [{"emb": e, "emb/Adagrad": e.slot("Adagrad", opt.init_acc)} for e in (a, b)]
    for e in (a, b):
        e.track_updates()
        e.track_removals()
    return a, b, opt, va, vb


@pytest.mark.parametrize("with_step", [False, True], ids=["no_step", "global_step"])
def test_delta_bytes_equal_twin(dr, uni, tmp_path, with_step):
    from deeprec_amd import checkpoint as ck
    a, b, opt, va, vb = trainer_pair(dr)
    rng = np.random.default_rng(12)
    gs = 0
    for rnd in range(3):
        for _ in range(5):
            gs += 1
            keys = rng.choice(uni, 260)
            for e in (a, b):
                train(dr, opt, e, keys, gs)
            if gs % 2 == 0:
                a.demote_to(int(rng.integers(200, 401)), compact=bool(gs % 4))
        gone = rng.choice(uni, 80, replace=False)
        assert a.remove(T(gone)) == b.remove(T(gone)) > 0
        if rnd == 1:        # a demotion between the last step and the save
            assert a.demote_to(200, compact=False) > 0
        assert a.tier_count() > 0
        assert a.updated_count() >= a.export_updated()[0].numel() > 100
        step = gs if with_step else None
        pa = ck.save_incremental(str(tmp_path / ("tiered_%d" % rnd)), va, global_step=step)
        pb = ck.save_incremental(str(tmp_path / ("twin_%d" % rnd)), vb, global_step=step)
        for ext in (".index", ".data-00000-of-00001"):
            assert filecmp.cmp(pa + ext, pb + ext, shallow=False), (rnd, ext)
        assert int(a.total_count()[0]) <= 300
        for e in (a, b):    # cleared on both tiers
            assert e.export_updated()[0].numel() == 0 and e.export_removed().numel() == 0
        r = ck.BundleReader(pa)
        n_up = r.dtype_and_shape("emb-sparse_incr_keys")[1][0]
        n_rm = r.dtype_and_shape("emb-sparse_incr_removed_keys")[1][0]
        assert n_up > 100 and n_rm > 10, (n_up, n_rm)
    dr.status_check()


# ---------------------------------------------------------------------------
# 4. a replica chain fed by a tiered trainer's deltas
# ---------------------------------------------------------------------------
def test_replica_chain(dr, uni, tmp_path):
    from deeprec_amd import checkpoint as ck
    pos = uni[uni >= 0]                                     # (the format drops negative keys)
    a, _, opt, va, _ = trainer_pair(dr, max_keys=400)
    rng = np.random.default_rng(21)
    gs = 0
    for _ in range(5):
        gs += 1
        train(dr, opt, a, rng.choice(pos, 260), gs)
    full = ck.save(str(tmp_path / "full"), va, global_step=gs)
    assert a.tier_count() > 0
    r1, r2 = make(dr, False), make(dr, True, max_keys=250)
    v1, v2 = [{"emb": e, "emb/Adagrad": e.slot("Adagrad", opt.init_acc)} for e in (r1, r2)]
    ck.restore(full, v1)
    ck.restore(full, v2)
    seen_tier_removal = 0
    for rnd in range(4):
        for _ in range(3):
            gs += 1
            train(dr, opt, a, rng.choice(pos, 260), gs)
            if gs % 2:
                a.demote_to(int(rng.integers(200, 401)), compact=False)
        t0 = a.tier_count()
        a.remove(T(rng.choice(pos, 60, replace=False)))
        seen_tier_removal += t0 - a.tier_count()
        p = ck.save_incremental(str(tmp_path / ("delta_%d" % rnd)), va, global_step=gs)
        ck.restore_incremental(p, v1, compact=True)
        ck.restore_incremental(p, v2, compact=True)
        for name in va:
            want = tup(va[name].export())
            same(tup(v1[name].export()), want, "round %d: %s of the untiered replica" % (rnd, name))
            same(tup(v2[name].export()), want, "round %d: %s of the tiered replica" % (rnd, name))
        assert r1.rows_allocated() == int(r1.total_count()[0])
        assert int(r2.total_count()[0]) <= 250 and r2.tier_count() > 0
        assert int(a.total_count()[0]) <= 400
    assert seen_tier_removal > 0
    dr.status_check()


# ---------------------------------------------------------------------------
# 5. the default is unchanged
# ---------------------------------------------------------------------------
def test_default_still_refuses(dr, uni):
    from deeprec_amd import checkpoint as ck
    a = make(dr, True, incremental=False, max_keys=200)
    slot = a.slot("Adagrad", 0.1)
    assert a.tiered
    for call in (a.track_updates, a.track_removals, slot.track_updates,
                 lambda: ck.save_incremental("/nonexistent/never_written", {"emb": a}, 3),
                 lambda: ck.restore_incremental("/nonexistent/never_read", {"emb": a})):
        with pytest.raises(dr.InvalidArgumentError, match="host-DRAM tier"):
            call()
    b = make(dr, True, max_keys=200)
    b.track_updates()
    b.track_removals()
    b.sparse_read(T(uni[:600]))
    b.mark_updated(T(uni[:500]))
    assert b.demote_to() == 400 and b.tier_count() == 400
    n = b.export_updated()[0].numel()
    assert n == 500 and b.updated_count() >= n
    b.track_updates(False)                                  # off and on: no stale flags
    b.track_updates()
    assert b.updated_count() == 0 and b.export_updated()[0].numel() == 0
    dr.status_check()
