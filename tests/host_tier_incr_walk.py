"""The walk of tests/test_gpu_host_tier_incr.py::test_tiered_incremental_walk
and a dict model of a tiered trainer that tracks updates and logs removals
(DESIGN section 17): which keys HBM holds, which the host tier holds, which
are marked as updated, and the removal log.

Not a test module and numpy only.  The model generates the seeded operation
lists (it steers by its own state), tests/test_host_tier_incr_walk_model.py
asserts on the CPU that every seed the GPU test uses makes the events happen
that the feature is about, and the GPU test replays the same lists on an
opted-in tiered EV and its untiered, unbudgeted twin, comparing both with the
model after every operation.  It extends the idea of tests/host_tier_walk.py.

Each transition cites the rule it restates (`kv` is
deeprec-1_amd/deeprec_amd/kv_variable_ops.py, `ev.hip` is
deeprec-1_amd/csrc/ev.hip, `lifecycle` is tests/ev_lifecycle.py, whose model
the GPU lifecycle test holds against the same code).
"""
import collections

import numpy as np

import ev_lifecycle as L

DIM = L.DIM
STEPS_TO_LIVE = 6
N_OPS = 120
MIN_ROWS = L.MIN_ROWS       # capacity=1: 1 024 rows
BUDGETS = (200, 400)        # demote_to(n), n drawn from this range
MAX_BATCH = 300
NEED = 5                    # each event of the list below, at least this often per seed

Case = collections.namedtuple("Case", "seed opt policy by_row filter_freq")
# opt: sgd | adagrad (the slot column); policy: lru | lfu; by_row: track_updates(by_row=True)
# and a row-recording forward; filter_freq 1: a Counter filter, which "lfu" needs
CASES = [
    Case(31, "adagrad", "lru", False, 0),
    Case(34, "sgd", "lru", True, 0),
    Case(33, "adagrad", "lfu", False, 1),
]

EVENTS = (
    "tier_export",      # 1. marked, demoted, exported from the tier while still there
    "carried_back",     # 2. marked, demoted, promoted again by a plain lookup, exported from HBM
    "cleared_demoted",  # 3. marked before a clear, demoted after it, absent from the next delta
    "tier_removed",     # 4. removed by remove() while in the tier
    "tier_aged",        # 5. aged out by shrink() while in the tier
    "recreated_marked",  # 6. evicted, re-created and updated again within one delta interval
)


def case_id(case):
    return "%s-%s-%s-seed%d" % (case.opt, case.policy, "byrow" if case.by_row else "bykey",
                                case.seed)


def universe(seed):
    """About 1 500 int64 keys of lifecycle.universe(seed): -1, 0, INT64_MIN,
    INT64_MAX, the 500 random keys of both signs and 28 clustered groups, each
    sharing a home line (groups[0] on the last one)."""
    u = L.universe(seed)
    keys = np.concatenate([u.keys[:4], u.keys[4:504]] + list(u.groups[:28]))
    assert np.unique(keys).size == keys.size and 1300 <= keys.size <= 1700
    assert set(keys[:4].tolist()) == {-1, 0, L.I64MIN, L.I64MAX}
    return keys, u.groups[:28]


class Key(object):
    """One key of the model: version, freq, the first-touch bits of the
    primary (c0) and the slot column (c1), and `carried`: it was marked when it
    was demoted (only meaningful in the tier)."""
    __slots__ = ("ver", "freq", "c0", "c1", "carried")

    def __init__(self, ver, freq, c0, c1):
        self.ver, self.freq, self.c0, self.c1, self.carried = ver, freq, c0, c1, False


class Model(object):
    def __init__(self, case):
        self.case = case
        self.filter = case.filter_freq > 0
        self.slot = case.opt == "adagrad"
        self.hbm, self.tier = {}, {}
        self.marked, self.log = set(), set()
        self.tracking = True
        self.gs = 0
        self.top = 0                # rows_allocated() of the tiered EV
        self.peak_top_flagged = 0   # the most rows allocated while the tier held a marked key
        self.stale = set()          # marked at the last clear, not marked again since
        self.gone = set()           # removed / aged out since the last clear
        self.stats = collections.Counter()

    # -- helpers ------------------------------------------------------------
    def _promote(self, keys):
        """kv.promote_grouped: the batch's keys the tier holds return to HBM as
        they were (version, freq, first-touch bits), each on a new row; with
        tracking on, its update bit with it (dr_ev_promote).  Returns them."""
        back = [k for k in dict.fromkeys(keys) if k in self.tier]
        for k in back:
            self.hbm[k] = self.tier.pop(k)
        self.top += len(back)
        return back

    def _sight(self, keys):
        """lifecycle.Model._sight: a lookup creates the absent keys (version 0;
        without a filter the primary column is touched, a Counter filter with
        filter_freq 1 counts the first sighting and admits at the second)."""
        for k in keys:
            r = self.hbm.get(k)
            if r is None:
                self.hbm[k] = Key(0, 1 if self.filter else 0, not self.filter, False)
                self.top += 1
            elif not r.c0:
                r.c0 = True

    def _drop(self, k, route):
        """remove() / shrink() on either tier: the key leaves the model and the
        updated set, and the removal log gets it (kv.EmbeddingVariable.remove /
        .shrink with dr_ev_log_removed for the tier's side)."""
        if k in self.tier:
            del self.tier[k]
            self.stats["tier_" + route] += 1
        else:
            del self.hbm[k]
        self.marked.discard(k)
        self.stale.discard(k)
        self.log.add(k)
        self.gone.add(k)

    def _mark(self, k):
        self.marked.add(k)
        self.stale.discard(k)

    # -- transitions --------------------------------------------------------
    def apply(self, op):
        ret = getattr(self, "_op_" + op["op"])(op)
        if any(k in self.marked for k in self.tier):
            self.peak_top_flagged = max(self.peak_top_flagged, self.top)
        return ret

    def _op_lookup(self, op):
        keys = op["keys"].tolist()
        for k in self._promote(keys):
            # the update bit came back in colmask bit 16: nothing else marks a key
            # that a plain lookup promotes
            if k in self.marked and self.hbm[k].carried:
                self.stats["carried_back"] += 1
        self._sight(keys)

    def _op_train(self, op):
        keys = op["keys"].tolist()
        self.gs = op["gs"]
        self._promote(keys)
        self._sight(keys)
        for k in dict.fromkeys(keys):
            r = self.hbm[k]
            # the apply admits a counted key, stamps version = gs and touches the slot
            # column; apply_gradients marks the gradient's indices (lifecycle._op_train)
            r.c0 = True
            r.c1 = r.c1 or self.slot
            r.ver = op["gs"]
            if self.tracking:
                if k in self.gone and k not in self.marked:
                    self.stats["recreated_marked"] += 1
                self._mark(k)

    def _op_mark(self, op):
        """Public mark_updated: absent keys and keys whose primary row is
        untouched are ignored, in HBM (mark_updated docstring) and in the tier
        (dr_host_tier_or_bits, require = the primary bit); nothing while
        tracking is off."""
        if not self.tracking:
            return
        for k in op["keys"].tolist():
            r = self.hbm.get(k) or self.tier.get(k)
            if r is not None and r.c0:
                if k in self.tier:
                    self.stats["tier_marked"] += 1
                    r.carried = True
                self._mark(k)

    def victims(self, n, policy):
        """shrink_to docstring: the first N - n keys of HBM by (version, key) or
        (freq, key); every key in the map counts, admitted or not."""
        keys = np.array(sorted(self.hbm), np.int64)
        m = np.array([getattr(self.hbm[k], "ver" if policy == "lru" else "freq")
                      for k in keys.tolist()], np.int64)
        assert (m >= 0).all()       # (no version -1 in this walk: nothing is inserted)
        return keys[np.lexsort((keys, m))[:max(keys.size - n, 0)]].tolist()

    def _op_demote(self, op):
        """demote_to(n, policy, compact): the victims move to the tier with
        their state; they stay in the model, in the updated set (bit 16 of
        colmask) and out of the removal log."""
        v = self.victims(op["n"], self.case.policy)
        for k in v:
            r = self.hbm.pop(k)
            r.carried = k in self.marked
            self.tier[k] = r
            if r.carried:
                self.stats["tier_export"] += 1
            elif k in self.stale:
                self.stats["cleared_demoted"] += 1
        if op["compact"]:
            self.top = len(self.hbm)    # compact(): rows_allocated() == total_count()
        return len(v)

    def _op_remove(self, op):
        gone = [k for k in dict.fromkeys(op["keys"].tolist()) if k in self.hbm or k in self.tier]
        for k in gone:
            self._drop(k, "removed")
        return len(gone)

    def _op_shrink(self, op):
        """The age rule on both tiers (lifecycle.Model._shrink, HostTier::shrink)."""
        n = 0
        for d in (self.hbm, self.tier):
            for k in list(d):
                assert d[k].ver != -1
                if op["gs"] - d[k].ver > STEPS_TO_LIVE:
                    self._drop(k, "aged")
                    n += 1
        return n

    def _op_clear(self, op):
        """clear_updated on both tiers; the removal log stays."""
        self.stale = set(self.marked)
        self.marked.clear()
        self.gone.clear()
        self.stats["clears"] += 1

    def _op_track_off(self, op):
        """track_updates(False): the bitmap goes, and the store's flags with it."""
        self._op_clear(op)
        self.tracking = False

    def _op_track_on(self, op):
        self.tracking = True

    # -- observables --------------------------------------------------------
    def observe(self):
        both = dict(self.hbm)
        both.update(self.tier)
        k0 = sorted(k for k, r in both.items() if r.c0)
        k1 = sorted(k for k, r in both.items() if r.c0 and r.c1)
        o = {
            "keys": np.array(k0, np.int64),
            "versions": np.array([both[k].ver for k in k0], np.int64),
            "slot_keys": np.array(k1, np.int64),
            "removed": np.array(sorted(self.log), np.int64),
            "hbm_count": len(self.hbm),
            "tier_count": len(self.tier),
            "rows": self.top,
        }
        if self.tracking:
            o["updated"] = np.array([k for k in k0 if k in self.marked], np.int64)
            o["slot_updated"] = np.array([k for k in k1 if k in self.marked], np.int64)
        return o


def replay_info(case, ops, i):
    last = ["  #%d %s" % (j, L.describe(ops[j])) for j in range(max(0, i - 10), i + 1)]
    return "walk %s (seed %d) failed at operation #%d; the last operations were\n%s" % (
        case_id(case), case.seed, i, "\n".join(last))


# ---------------------------------------------------------------------------
# The generator
# ---------------------------------------------------------------------------
class _Gen(object):
    def __init__(self, case, n_ops):
        self.case, self.n_ops = case, n_ops
        self.rng = np.random.default_rng([case.seed, 2])
        self.keys, self.groups = universe(case.seed)
        self.m = Model(case)
        self.ops = []

    def emit(self, **op):
        self.ops.append(op)
        self.m.apply(op)

    def pick(self, pool, n):
        pool = np.array(sorted(pool), np.int64)
        n = min(n, pool.size)
        return self.rng.choice(pool, n, replace=False) if n else pool[:0]

    def batch(self, n, tier_share, dups=True):
        """n keys: a share from the tier (marked ones first), the rest from the
        whole universe; now and then a clustered group and the special keys."""
        rng, m = self.rng, self.m
        nt = int(n * tier_share)
        flagged = [k for k in m.tier if k in m.marked]
        parts = [self.pick(flagged, nt // 2), self.pick(m.tier, nt - nt // 2),
                 rng.choice(self.keys, n - nt, replace=False)]
        if rng.random() < 0.3:
            parts.append(self.groups[int(rng.integers(0, len(self.groups)))])
        if rng.random() < 0.4:
            parts.append(self.keys[:4])
        keys = np.unique(np.concatenate(parts))
        keys = rng.permutation(keys)[:MAX_BATCH]
        if dups and keys.size > 8:
            keys = rng.permutation(np.concatenate([keys, rng.choice(keys, keys.size // 8)]))
        return keys[:MAX_BATCH].astype(np.int64)

    def step(self):
        rng, m = self.rng, self.m
        w = dict(train=30, lookup=12, demote=18, remove=8, shrink=5, mark=8, clear=6, track=2)
        if not m.tracking:      # a few operations with tracking off (two at least), then on again
            off = max(i for i, o in enumerate(self.ops) if o["op"] == "track_off")
            w = dict(train=4, demote=4, mark=2, track=6 if len(self.ops) - off > 2 else 0)
        if len(m.hbm) < BUDGETS[0]:
            w.update(demote=0)
        names = sorted(w)
        p = np.array([w[n] for n in names], float)
        name = names[int(rng.choice(len(names), p=p / p.sum()))]
        if name == "train":
            keys = self.batch(int(rng.integers(120, 260)), 0.15)
            self.emit(op="train", keys=keys, gs=m.gs + 1,
                      grads=rng.integers(-2, 3, (np.unique(keys).size, DIM)).astype(np.float32))
        elif name == "lookup":
            self.emit(op="lookup", keys=self.batch(int(rng.integers(40, 160)), 0.6))
        elif name == "demote":
            self.emit(op="demote", n=int(rng.integers(BUDGETS[0], BUDGETS[1] + 1)),
                      compact=bool(rng.random() < 0.5))
        elif name == "remove":
            keys = np.concatenate([self.pick(m.tier, 25), self.pick(m.hbm, 25),
                                   rng.choice(self.keys, 15)])
            self.emit(op="remove", keys=rng.permutation(keys).astype(np.int64))
        elif name == "shrink":
            self.emit(op="shrink", gs=m.gs)
        elif name == "mark":
            keys = np.concatenate([self.pick(m.tier, 30), self.pick(m.hbm, 30),
                                   rng.choice(self.keys, 20)])
            self.emit(op="mark", keys=rng.permutation(keys).astype(np.int64))
        elif name == "clear":
            self.emit(op="clear")
        elif name == "track":
            self.emit(op="track_off" if m.tracking else "track_on")

    def run(self):
        while len(self.ops) < self.n_ops:
            self.step()
        if not self.m.tracking:
            self.emit(op="track_on")
        return self.ops


def generate(case, n_ops=N_OPS):
    """The walk of `case`: about n_ops operations, each a dict {"op": name, ...}."""
    return _Gen(case, n_ops).run()


def replay(case, ops):
    m = Model(case)
    for op in ops:
        m.apply(op)
    return m
