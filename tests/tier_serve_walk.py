"""A seeded serving walk over a tiered Counter EmbeddingVariable (DESIGN section
19) and a dict model of where each key lives: rounds of training, a demotion
of everything HBM holds, a little more training (which promotes what it
names), then pooled read-only serving batches that mix ids the tier serves,
ids the tier holds but the Counter rule keeps at the default, ids HBM holds
and ids nobody has seen.

Not a test module and numpy only: tests/test_tier_serve_walk_model.py checks on
the CPU that the walk's inputs are not vacuous, tests/test_gpu_tier_serve.py
runs the same operations on a tiered EV and its untiered, unbudgeted twin.

The model is exact about places because every demotion is demote_to(0): a
training lookup brings the keys it names into HBM (created or promoted), the
demotion moves all of HBM to the tier.  About admission it only claims what
holds however a sighting is counted: a key trained in >= 2 steps is served
(freq >= 2, touched by the apply), a key sighted once and never trained is
not (freq 1 < FILTER_FREQ); a key trained in exactly one step is left
unclassified.
"""
import numpy as np

import ev_lifecycle as L

SEEDS = [31, 32, 33, 34, 35]
ROUNDS = 4
FILTER_FREQ = 2
BAGS = 64               # bags per serving batch
SPECIAL = np.array([-1, 0, L.I64MIN, L.I64MAX], np.int64)
COMBINERS = ("sum", "mean", "sqrtn")
# classes of a served id, by the model
SERVED, FILTERED, NEVER, HBM, OTHER = range(5)


class Model(object):
    def __init__(self):
        self.hbm, self.tier = {}, {}    # key -> training steps that named it (0: sighted once)

    def touch(self, keys, trained):
        for k in np.unique(keys).tolist():
            n = self.tier.pop(k) if k in self.tier else self.hbm.get(k, 0)
            self.hbm[k] = n + (1 if trained else 0)

    def demote_all(self):
        self.tier.update(self.hbm)
        self.hbm = {}

    def classify(self, k):
        if k in self.tier:
            n = self.tier[k]
            return SERVED if n >= 2 else (FILTERED if n == 0 else OTHER)
        return HBM if k in self.hbm else NEVER

    def tier_keys(self, cls):
        return np.array(sorted(k for k in self.tier if self.classify(k) == cls), np.int64)


def _bags(rng, ids_of):
    """BAGS bags of 0..5 ids: (indices [nnz, 2], values [nnz], width)."""
    lens = rng.integers(0, 6, BAGS)
    lens[rng.integers(0, BAGS)] = 0
    lens[rng.integers(0, BAGS)] = 5
    rows = np.repeat(np.arange(BAGS), lens)
    cols = np.concatenate([np.arange(n) for n in lens]).astype(np.int64)
    vals = ids_of(int(lens.sum()))
    # repeats inside a bag: the second id of every long bag is its first again
    start = np.cumsum(lens) - lens
    for b in np.nonzero(lens >= 4)[0]:
        vals[start[b] + 1] = vals[start[b]]
    return np.stack([rows, cols], 1).astype(np.int64), vals, 5


def walk(seed):
    """The operations of one walk, in order, as dicts:
      {"op": "train", "keys", "step"}   sparse_read + SGD on the distinct keys
      {"op": "sight", "keys"}           one sparse_read of distinct, fresh keys
      {"op": "demote"}                  demote_to(0)
      {"op": "serve", "kind": "onehot" | "bags", "combiner", "indices", "values",
       "width", "classes"}              one pooled read-only lookup
      {"op": "end", "tier"}             the keys the tier holds at the end, ascending
    and the model's counts of served ids by class."""
    uni = L.universe(seed)
    rng = np.random.default_rng([seed, 19])
    pool = rng.permutation(uni.keys[~np.isin(uni.keys, SPECIAL)])
    never, pool = pool[:300], pool[300:]
    at = [0]

    def fresh(n):
        out = pool[at[0]:at[0] + n]
        at[0] += n
        assert out.size == n, "the universe ran out of fresh keys"
        return out

    m = Model()
    ops, counts = [], np.zeros(5, np.int64)
    step = 0
    for rnd in range(ROUNDS):
        known = np.array(sorted(list(m.hbm) + list(m.tier)), np.int64)
        cand = fresh(220)
        if known.size:
            cand = np.concatenate([cand, rng.choice(known, 80, replace=False)])
        for _ in range(3):
            keys = rng.choice(cand, 300)
            if rnd == 0:
                keys = np.concatenate([keys, SPECIAL])
            ops.append({"op": "train", "keys": keys.astype(np.int64), "step": step})
            m.touch(keys, True)
            step += 1
        once = fresh(30)
        ops.append({"op": "sight", "keys": once})
        m.touch(once, False)
        ops.append({"op": "demote"})
        m.demote_all()
        back = rng.choice(np.array(sorted(m.tier), np.int64), 100, replace=False)
        back = back[~np.isin(back, SPECIAL)]
        back = back[[m.tier[k] > 0 for k in back.tolist()]]     # (a sighted-once key stays one)
        ops.append({"op": "train", "keys": np.concatenate([back, back[:20]]), "step": step})
        m.touch(back, True)
        step += 1
        src = {SERVED: m.tier_keys(SERVED), FILTERED: m.tier_keys(FILTERED), NEVER: never,
               HBM: np.array(sorted(m.hbm), np.int64), OTHER: m.tier_keys(OTHER)}
        mix = [(SERVED, 0.48), (FILTERED, 0.13), (NEVER, 0.13), (HBM, 0.18), (OTHER, 0.08)]

        def ids_of(n):
            parts = [rng.choice(src[c], max(int(round(n * f)), 1)) for c, f in mix if src[c].size]
            ids = np.concatenate(parts + [SPECIAL])
            return rng.permutation(ids)[:n] if ids.size >= n else \
                np.concatenate([ids, rng.choice(src[SERVED], n - ids.size)])

        for s in range(4):
            if s % 2 == 0:
                vals = ids_of(BAGS)
                ind = np.stack([np.arange(BAGS), np.zeros(BAGS, np.int64)], 1).astype(np.int64)
                op = {"op": "serve", "kind": "onehot", "combiner": "sum", "indices": ind,
                      "values": vals, "width": 1}
            else:
                ind, vals, width = _bags(rng, ids_of)
                op = {"op": "serve", "kind": "bags", "combiner": COMBINERS[(rnd + s // 2) % 3],
                      "indices": ind, "values": vals, "width": width}
            op["values"] = op["values"].astype(np.int64)
            op["classes"] = np.array([m.classify(k) for k in op["values"].tolist()], np.int64)
            counts += np.bincount(op["classes"], minlength=5)
            ops.append(op)
    ops.append({"op": "end", "tier": np.array(sorted(m.tier), np.int64)})
    return ops, counts
