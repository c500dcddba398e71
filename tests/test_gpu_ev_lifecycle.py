"""The EmbeddingVariable lifecycle under a long, unscripted mix of operations.

A deterministic random walk (tests/ev_lifecycle.py: about 160 operations over
about 2 500 keys, batches of 1-400) runs on three EVs and is checked after
EVERY operation:

  A  the EV under stress: capacity=1 (1 024 rows / 2 048 slots, so it grows and
     rehashes), int64 keys, dim 8, steps_to_live 8, update tracking and the
     removal log on from the start; marks by row, removes in one call, takes
     the key budget through shrink_to, compacts and reserves;
  B  its twin at the default capacity (it never grows, compacts or reserves),
     which receives every logical operation by the plain route: marks by key,
     the same removal split over three calls, remove(numpy's victims) for the
     budget, shrink + clear for a sync;
  R  a replica restored once from a full save and then fed by save_incremental
     / restore_incremental(compact=True) alone;
  M  the dict model (ev_lifecycle.Model), M_R for the replica.

A == B bit for bit in every column and observable; A == M in the key set, the
updated and logged keys, the row counts and -- in the SGD cases, where the
model's arithmetic is exact -- the value bits and versions; a read-only lookup
or find changes nothing; after every sync R == M_R and R serves what A serves
for every non-negative key of the universe.

Two configurations differ from a plain EV because the library refuses the
plain one: shrink_to(policy="lfu") needs the freq column a Counter filter
keeps, so the lfu case runs CounterFilter(filter_freq=1), and the sparse apply
kernels take float rows only, so the float64 case trains by upsert of the SGD
step computed in float64 (values, version = global step, then the mark).

A failing walk names its seed, the operation and the ten before it; replay it
with ev_lifecycle.generate(case)[:i + 1].

Wall time per case on an MI355X (the whole walk with all checks, 160 operations):
  float32-sgd-lru-seed11      0.82 s (1.7 s as the first test of a process)
  float32-adagrad-lru-seed12  0.88 s
  bfloat16-sgd-lru-seed13     0.80 s
  float32-sgd-lfu-seed14      0.99 s
  float64-sgd-lru-seed15      0.83 s
  float32-sgd-lru-seed16      0.81 s
  float32-sgd-lru-seed17      0.79 s

The walks found three bugs, each pinned below by the shortest sequence that
showed it: the first update of a key a Counter filter admits in the apply was
not marked (training.py), a float64 EV's checkpoint scrambled its rows, and a
bf16 EV could not be saved at all (checkpoint.py).
"""
import time

import numpy as np
import pytest
import torch

import ev_lifecycle as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I64MAX = np.iinfo(np.int64).max
TORCH_DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float64": torch.float64}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _bits(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy()
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _snap(ev, updated=False):
    k, v, ve, fr = ev.export_updated() if updated else ev.export()
    return k.cpu().numpy(), _bits(v), ve.cpu().numpy(), fr.cpu().numpy()


def _same(got, ref, what):
    assert got.keys() == ref.keys(), what
    for name in got:
        g, r = got[name], ref[name]
        if not isinstance(g, tuple):
            g, r = (g,), (r,)
        for i, (x, y) in enumerate(zip(g, r)):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape, \
                "%s: %s[%d] is %s %s against %s %s" % (what, name, i, x.dtype, x.shape, y.dtype,
                                                       y.shape)
            assert np.array_equal(x, y), "%s: %s[%d] differs, first at %s" % (
                what, name, i, np.argwhere(x != y)[0].tolist())


class Walk(object):
    """The three EVs of one walk: the `subject` of ev_lifecycle.run_walk."""

    def __init__(self, dr, ck, case, tmp_path):
        self.dr, self.ck, self.case, self.dir = dr, ck, case, tmp_path
        self.uni = L.universe(case.seed)
        self.sample_t = _t(self.uni.sample)
        self.nonneg_t = _t(self.uni.keys[self.uni.keys >= 0])
        self.filter = L.has_filter(case)
        opt = dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(filter_freq=1)) \
            if self.filter else None

        def ev(tag, **kw):
            return dr.EmbeddingVariable("lifecycle_%s_%s" % (L.case_id(case), tag), L.DIM,
                                        L.DEFAULT, steps_to_live=L.STEPS_TO_LIVE, ev_option=opt,
                                        device=DEV, value_dtype=TORCH_DT[case.dtype], **kw)

        self.A, self.B, self.R = ev("A", capacity=1), ev("B"), ev("R", capacity=1)
        self.colsA, self.colsB, self.colsR = [self.A], [self.B], [self.R]
        if case.opt == "adagrad":
            self.opt = dr.AdagradOptimizer(L.LR)
            for cols in (self.colsA, self.colsB, self.colsR):   # the slot the optimizer creates
                cols.append(cols[0].slot("Adagrad", self.opt.init_acc))
        else:
            self.opt = dr.GradientDescentOptimizer(L.LR)
        names = ["emb", "emb/Adagrad"]
        self.varsA = dict(zip(names, self.colsA))
        self.varsR = dict(zip(names, self.colsR))
        for p in (self.A, self.B):
            p.track_updates()
            p.track_removals()
        self.cap = lambda e: dr._lib.lib().dr_ev_row_capacity(e.handle)
        self.cap0 = (self.cap(self.A), self.cap(self.B))
        assert self.cap0[0] == L.MIN_ROWS
        self.reclaimed = 0
        self.n = 0
        self.sa, self.sb = self._state(self.colsA), self._state(self.colsB)

    # -- observables -----------------------------------------------------------
    def _state(self, cols):
        """`shared`: everything a twin must agree on, bit for bit; `own`: what
        belongs to one EV (row indices, row counts) but must survive a read."""
        p = cols[0]
        shared = {"count": int(p.total_count()[0]), "removed": p.export_removed().cpu().numpy(),
                  "meta": p.key_meta(self.uni.sample)}
        for i, c in enumerate(cols):
            shared["export%d" % i] = _snap(c)
            shared["updated%d" % i] = _snap(c, True)
            shared["read%d" % i] = _bits(c.sparse_read(self.sample_t, read_only=True))
        own = {"rows": p.rows_allocated(), "updated_count": p.updated_count(),
               "removed_count": p.removed_count(),
               "find": p.find(self.sample_t).cpu().numpy()}
        return shared, own

    def observe(self, sample):
        (s, own), (_, own_b) = self.sa, self.sb
        k, v, ve, fr = s["export0"]
        o = {"keys": k, "values": v, "versions": ve, "freqs": fr, "count": s["count"],
             "updated": s["updated0"][0], "removed": s["removed"], "rows": own["rows"],
             "twin_rows": own_b["rows"], "sample_has_row": s["meta"][2],
             "sample_version": s["meta"][1]}
        # the count of marked rows is an upper bound (updated_count docstring)
        assert own["updated_count"] >= o["updated"].size
        assert own["removed_count"] >= o["removed"].size
        assert ((own["find"] >= 0) == o["sample_has_row"]).all()
        return o

    def observe_replica(self):
        k, v, _, _ = _snap(self.R)
        return {"keys": k, "values": v, "count": int(self.R.total_count()[0]),
                "rows": self.R.rows_allocated()}

    # -- one operation ---------------------------------------------------------------
    def apply(self, op):
        before = (self.sa, self.sb)
        ret = getattr(self, "_op_" + op["op"])(op)
        self.n += 1
        self.sa, self.sb = self._state(self.colsA), self._state(self.colsB)
        _same(self.sa[0], self.sb[0], "A against its twin B")
        if op["op"] == "lookup_ro":         # state before == state after, row indices included
            for new, old, who in ((self.sa, before[0], "A"), (self.sb, before[1], "B")):
                _same(new[0], old[0], "%s after a read-only lookup" % who)
                _same(new[1], old[1], "%s after a read-only lookup" % who)
        return ret

    def _both(self, fn):
        a, b = fn(self.A), fn(self.B)
        return a, b

    def _op_lookup(self, op):
        k = _t(op["keys"])
        a, b = self._both(lambda e: _bits(e.sparse_read(k)))
        assert np.array_equal(a, b), "the rows lookup returned differ between A and B"

    def _op_lookup_ro(self, op):
        k = _t(op["keys"])
        a, b = self._both(lambda e: _bits(e.sparse_read(k, read_only=True)))
        assert np.array_equal(a, b), "the rows a read-only lookup returned differ"
        fa, fb = self._both(lambda e: e.find(k).cpu().numpy())
        assert np.array_equal(fa >= 0, fb >= 0), "find() differs between A and B"

    def _op_train(self, op):
        keys, gs = op["keys"], op["gs"]
        k = _t(keys)
        outs = []
        for ev in (self.A, self.B):
            out = ev.sparse_read(k)
            outs.append(_bits(out))
            if self.case.dtype != "float64":
                ev.pending_grads.append(self.dr.IndexedSlices(_t(op["grads"]), k))
                self.opt.apply_gradients([ev], global_step=gs)
                assert not ev.pending_grads
                continue
            # a float64 EV: the SGD step in float64 on the host, written by upsert
            u, first, inv = np.unique(keys, return_index=True, return_inverse=True)
            g = np.zeros((u.size, L.DIM), np.float64)
            np.add.at(g, inv, op["grads"].astype(np.float64))
            new = out.cpu().numpy()[first] - L.LR * g
            ev.upsert(_t(u), _t(new), _t(np.full(u.size, gs, np.int64)))
            if ev is self.A:
                ev.mark_updated_rows(ev.find(_t(u)))
            else:
                ev.mark_updated(_t(u))
        assert np.array_equal(outs[0], outs[1]), "the rows the training lookup returned differ"

    def _put(self, op):
        ver = None if op["versions"] is None else _t(op["versions"])
        frq = None if op["freqs"] is None else _t(op["freqs"])
        for ev in (self.A, self.B):
            getattr(ev, op["op"])(_t(op["keys"]), _t(op["values"]), ver, frq)

    _op_insert = _op_upsert = _put

    def _op_mark(self, op):
        k = _t(op["keys"])
        self.A.mark_updated_rows(self.A.find(k))    # rows taken immediately before the call
        self.B.mark_updated(k)

    def _op_remove(self, op):
        got = self.A.remove(_t(op["keys"]))
        parts = np.array_split(op["keys"], 3)
        twin = sum(self.B.remove(_t(p)) for p in parts if p.size)
        assert got == twin, "remove() returned %d, the twin's three calls %d" % (got, twin)
        return got

    def _op_budget(self, op):
        n, policy = op["n"], op["policy"]
        k, _, ve, fr = _snap(self.B)
        if self.filter:
            # keys a Counter filter has counted but not admitted are live too and not
            # exported: every key in the map has freq >= 1
            rest = self.uni.keys[~np.isin(self.uni.keys, k)]
            f2, v2, _ = self.B.key_meta(rest)
            k = np.concatenate([k, rest[f2 >= 1]])
            ve, fr = np.concatenate([ve, v2[f2 >= 1]]), np.concatenate([fr, f2[f2 >= 1]])
        assert k.size == int(self.B.total_count()[0])
        m = np.where(ve == -1, I64MAX, ve) if policy == "lru" else fr
        victims = k[np.lexsort((k, m))[:max(k.size - n, 0)]]
        got = self.A.shrink_to(n, policy)
        twin = self.B.remove(_t(victims)) if victims.size else 0
        assert got == twin == victims.size, (got, twin, victims.size)
        return got

    def _op_shrink(self, op):
        a, b = self._both(lambda e: e.shrink(op["gs"]))
        assert a == b, "shrink() returned %d on A, %d on B" % (a, b)
        return a

    def _op_compact(self, op):
        got = self.A.compact()
        self.reclaimed += got
        assert self.A.rows_allocated() == int(self.A.total_count()[0])
        return got

    def _op_reserve(self, op):
        self.A.reserve(op["extra"])

    def _op_base(self, op):
        full = self.ck.save(str(self.dir / "full"), self.varsA, global_step=None)
        self.ck.restore(full, self.varsR)

    def _op_sync(self, op):
        gs = op["gs"]
        p = self.ck.save_incremental(str(self.dir / ("delta_%d" % self.n)), self.varsA,
                                     global_step=gs)
        self.ck.restore_incremental(p, self.varsR, compact=True)
        n = self.B.shrink(gs)
        self.B.clear_updated()
        self.B.clear_removed()
        assert self.R.rows_allocated() == int(self.R.total_count()[0])
        for a, r in zip(self.colsA, self.colsR):    # the replica serves what the trainer serves
            ra = _bits(a.sparse_read(self.nonneg_t, read_only=True))
            rr = _bits(r.sparse_read(self.nonneg_t, read_only=True))
            assert np.array_equal(ra, rr), \
                "%s: the replica serves other rows than the trainer, first for key %d" % (
                    a.name, self.uni.keys[self.uni.keys >= 0][np.argwhere(ra != rr)[0][0]])
        return n


# ---------------------------------------------------------------------------
# What the walks found, reduced to the shortest sequences that showed it
# ---------------------------------------------------------------------------
def test_counter_filter_admitting_step_is_marked():
    """The lfu walk, operations #0-#3 (insert, mark, full save, train): in a
    Counter-filter EV the apply admits a key whose freq has reached
    filter_freq, and the mark skips a key whose primary row is untouched --
    apply_gradients marked before the apply, so the key's first update was
    missing from export_updated and from the next delta."""
    import deeprec_amd as dr
    opt = dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(filter_freq=3))
    ev = dr.EmbeddingVariable("lifecycle_counter_mark", L.DIM, 0.5, steps_to_live=8,
                              ev_option=opt, capacity=1024, device=DEV)
    ev.track_updates()
    old = np.arange(100, 140, dtype=np.int64)               # admitted by the insert
    new = np.arange(-20, 20, dtype=np.int64)                # seen twice: one sighting short
    young = np.arange(1000, 1006, dtype=np.int64)           # seen once
    ev.insert(_t(old), _t(np.ones((old.size, L.DIM), np.float32)))
    for k in (new, new, young):
        ev.sparse_read(_t(k))
    assert ev.export()[0].numel() == old.size
    keys = np.concatenate([old[:10], new, young])
    ev.sparse_read(_t(keys))                                # the step's lookup: the third sighting
    ev.pending_grads.append(dr.IndexedSlices(_t(np.ones((keys.size, L.DIM), np.float32)),
                                             _t(keys)))
    dr.GradientDescentOptimizer(0.5).apply_gradients([ev], global_step=1)
    want = np.sort(np.concatenate([old[:10], new]))         # `young` is at freq 2: not admitted
    k, v, ve, fr = _snap(ev, True)
    np.testing.assert_array_equal(k, want)
    ref = np.where(np.isin(want, old)[:, None], 1.0 - 0.5, 0.5 - 0.5) * np.ones((1, L.DIM))
    np.testing.assert_array_equal(v, ref.astype(np.float32).view(np.uint32))
    assert (ve == 1).all() and (fr >= 3).all()
    assert not np.isin(young, ev.export()[0].cpu().numpy()).any()
    dr.status_check()


@pytest.mark.parametrize("dtype,dim", [("float64", 8), ("float64", 5), ("bfloat16", 8),
                                       ("bfloat16", 6)])
def test_checkpoints_carry_double_and_bf16_rows(dtype, dim, tmp_path):
    """The float64 and bf16 walks, operations #0-#2 (insert, mark, full save):
    the save packs rows by key % 1000 in 32-bit words and took a row for dim
    of them, so a restored float64 EV held other rows' halves; and the bundle
    had no way to write a bf16 tensor, so saving a bf16 EV raised.  A full
    save and a delta must carry both, bit for bit."""
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    rng = np.random.default_rng(dim)
    keys = np.unique(rng.integers(0, 2**62, 700).astype(np.int64))[:600]
    rng.shuffle(keys)
    if dtype == "float64":
        rows = lambda n: rng.standard_normal((n, dim)) * np.pi          # full 53-bit mantissas
    else:
        rows = lambda n: (rng.integers(-100, 101, (n, dim)) / 8.0).astype(np.float32)   # exact
    a, b = [dr.EmbeddingVariable("lifecycle_ck_%s_%d_%s" % (dtype, dim, t), dim, 0.5,
                                 steps_to_live=8, capacity=1024, device=DEV,
                                 value_dtype=TORCH_DT[dtype]) for t in "ab"]
    a.insert(_t(keys), _t(rows(keys.size)), _t(rng.integers(0, 5, keys.size).astype(np.int64)))
    ck.restore(ck.save(str(tmp_path / "full"), {"emb": a}), {"emb": b})
    _same({"export": _snap(b)}, {"export": _snap(a)}, "a restored %s EV" % dtype)
    a.track_updates()
    part = keys[:250]
    a.upsert(_t(part), _t(rows(part.size)), _t(np.full(part.size, 7, np.int64)))
    a.mark_updated(_t(part))
    ck.restore_incremental(ck.save_incremental(str(tmp_path / "delta"), {"emb": a}), {"emb": b})
    sa = _snap(a)
    assert (sa[2][np.isin(sa[0], part)] == 7).all()
    _same({"export": _snap(b)}, {"export": sa}, "a %s EV after a delta" % dtype)
    dr.status_check()


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_lifecycle_walk(case, tmp_path):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    ops = L.generate(case)
    t0 = time.perf_counter()
    walk = Walk(dr, ck, case, tmp_path)
    m = L.run_walk(case, ops, walk)
    torch.cuda.synchronize()
    print("lifecycle walk %s: %d operations, %.2f s" % (L.case_id(case), len(ops),
                                                        time.perf_counter() - t0))
    # the walk went where it was meant to go: A grew, B did not, compactions moved rows
    assert walk.cap(walk.A) > L.MIN_ROWS
    assert walk.cap(walk.B) == walk.cap0[1]
    assert walk.reclaimed > 0
    assert m.stats["syncs"] >= 4 and m.stats["recreated"] >= 300
    dr.status_check()
