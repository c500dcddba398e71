"""The EV lifecycle walk without a GPU: the generator against the dict model.

Three things are pinned here, before anything runs on an EV:
  * the model itself, on hand-written timelines whose expected states are
    written out literally;
  * that the walks of exactly the cases tests/test_gpu_ev_lifecycle.py runs
    are not vacuous (conditions on the generator, asserted, not measured);
  * that the walk's comparison bites: a model with a planted lifecycle bug is
    caught by run_walk / compare within the first walk.
"""
import numpy as np
import pytest

import ev_lifecycle as L

F32 = L.Case(1, "float32", "sgd", "lru")


def _k(*a):
    return np.array(a, np.int64)


def _rows(*vals):
    return L.value_bits(np.array([[v] * L.DIM for v in vals], np.float32).reshape(-1, L.DIM),
                        "float32")


def _put(name, keys, vals, versions=None, freqs=None):
    return dict(op=name, keys=_k(*keys), values=np.array([[v] * L.DIM for v in vals], np.float32),
                versions=None if versions is None else _k(*versions),
                freqs=None if freqs is None else _k(*freqs))


def _state(m):
    o = m.observe(_k())
    return (o["keys"].tolist(), o["versions"].tolist(), o["updated"].tolist(),
            o["removed"].tolist(), o["count"], o["rows"])


# ---------------------------------------------------------------------------
# The model on hand-written timelines
# ---------------------------------------------------------------------------
def test_timeline_evict_recreate_mark_sync():
    m = L.Model(F32)
    assert m.apply(_put("insert", [5, 7, -3], [1.0, 2.0, 3.0], [0, 0, 0])) is None
    m.apply(dict(op="base"))
    assert sorted(m.rep) == [5, 7]                      # the format drops the negative key
    assert _state(m) == ([-3, 5, 7], [0, 0, 0], [], [], 3, 3)
    # 1: evict (an absent key and a duplicate among the keys)
    assert m.apply(dict(op="remove", keys=_k(7, 9, 5, 7))) == 2
    assert _state(m) == ([-3], [0], [], [5, 7], 1, 3)
    # 2: re-create: new keys with new rows, the default value, version 0; the log keeps them
    m.apply(dict(op="lookup", keys=_k(7, 5, 7)))
    assert _state(m) == ([-3, 5, 7], [0, 0, 0], [], [5, 7], 3, 5)
    np.testing.assert_array_equal(m.observe(_k())["values"], _rows(3.0, 0.5, 0.5))
    # 3: mark one of the two (and an absent key, which is ignored)
    m.apply(dict(op="mark", keys=_k(7, 11)))
    assert _state(m) == ([-3, 5, 7], [0, 0, 0], [7], [5, 7], 3, 5)
    # 4: sync: removals first, upserts second -- 7 arrives with its new row, 5 (re-created,
    # never updated) ends absent on the replica; marks and log are cleared
    assert m.apply(dict(op="sync", gs=0)) == 0
    assert _state(m) == ([-3, 5, 7], [0, 0, 0], [], [], 3, 5)
    r = m.observe_replica()
    assert r["keys"].tolist() == [7] and r["count"] == 1 and r["rows"] == 1
    np.testing.assert_array_equal(r["values"], _rows(0.5))
    # 5: compact gives the two dead rows back
    assert m.apply(dict(op="compact")) == 2
    assert _state(m) == ([-3, 5, 7], [0, 0, 0], [], [], 3, 3)


def test_timeline_version_minus_one():
    m = L.Model(F32)
    m.apply(_put("insert", [1, 2, 3], [1.0, 1.0, 1.0], [-1, 2, 0]))
    # 1: a training step at global step 11 stamps its key, marks it and moves its row
    m.apply(dict(op="train", keys=_k(3, 3), grads=np.ones((2, L.DIM), np.float32), gs=11))
    assert _state(m) == ([1, 2, 3], [-1, 2, 11], [3], [], 3, 3)
    np.testing.assert_array_equal(m.observe(_k())["values"], _rows(1.0, 1.0, 0.0))
    # 2: shrink(11): version -1 becomes 11 and stays; 11 - 2 > 8 goes
    assert m.apply(dict(op="shrink", gs=11)) == 1
    assert _state(m) == ([1, 3], [11, 11], [3], [2], 2, 3)
    # 3: 19 - 11 = 8 is not > 8
    assert m.apply(dict(op="shrink", gs=19)) == 0
    assert _state(m) == ([1, 3], [11, 11], [3], [2], 2, 3)
    # 4: 20 - 11 = 9 is: both go, the mark with its key
    assert m.apply(dict(op="shrink", gs=20)) == 2
    assert _state(m) == ([], [], [], [1, 2, 3], 0, 3)
    # 5: nothing is live: the compaction reclaims every row
    assert m.apply(dict(op="compact")) == 3
    assert _state(m) == ([], [], [], [1, 2, 3], 0, 0)


def test_timeline_budget_tie_broken_by_key():
    m = L.Model(F32)
    m.apply(_put("insert", [10, -5, 30, 20, -1], [1.0] * 5, [4, 4, 4, -1, 2]))
    # 1: by (version, key), -1 as the newest: (2, -1), (4, -5), (4, 10), (4, 30), (newest, 20)
    assert m.victims(3, "lru").tolist() == [-1, -5]
    assert m.apply(dict(op="budget", n=3, policy="lru")) == 2
    assert _state(m) == ([10, 20, 30], [4, -1, 4], [], [-5, -1], 3, 5)
    # 2: at the budget nothing changes
    assert m.apply(dict(op="budget", n=3, policy="lru")) == 0
    assert _state(m) == ([10, 20, 30], [4, -1, 4], [], [-5, -1], 3, 5)
    # 3: the tie at version 4 is cut by key; the unstamped key survives and is not rewritten
    assert m.apply(dict(op="budget", n=2, policy="lru")) == 1
    assert _state(m) == ([20, 30], [-1, 4], [], [-5, -1, 10], 2, 5)
    # 4: a victim comes back as a new key, version 0: now the coldest
    m.apply(dict(op="lookup", keys=_k(-5)))
    assert _state(m) == ([-5, 20, 30], [0, -1, 4], [], [-5, -1, 10], 3, 6)
    # 5
    assert m.apply(dict(op="budget", n=1, policy="lru")) == 2
    assert _state(m) == ([20], [-1], [], [-5, -1, 10, 30], 1, 6)


def test_timeline_lfu_and_the_counter_filter():
    """The lfu case's EV has CounterFilter(filter_freq=1): a key is in the map
    at its first sighting and admitted at the second, or by an insert."""
    m = L.Model(L.Case(1, "float32", "sgd", "lfu"))
    m.apply(_put("insert", [4, 6, 8], [1.0, 1.0, 1.0], None, [0, 3, 3]))
    m.apply(dict(op="lookup", keys=_k(9)))
    o = m.observe(_k(9, 4))
    assert o["keys"].tolist() == [4, 6, 8] and o["count"] == 4 and o["rows"] == 4
    assert o["freqs"].tolist() == [1, 3, 3]             # a freq below filter_freq is raised to it
    assert o["sample_has_row"].tolist() == [False, True]
    m.apply(dict(op="lookup", keys=_k(9)))
    assert m.observe(_k())["keys"].tolist() == [4, 6, 8, 9]
    assert m.victims(1, "lfu").tolist() == [4, 9, 6]    # (1, 4), (1, 9), (3, 6), (3, 8)


# ---------------------------------------------------------------------------
# The generator
# ---------------------------------------------------------------------------
def test_cases_cover_the_configurations():
    assert 6 <= len(L.CASES) <= 8 and len({c.seed for c in L.CASES}) == len(L.CASES)
    conf = [(c.dtype, c.opt, c.policy) for c in L.CASES]
    for want in (("float32", "sgd", "lru"), ("float32", "adagrad", "lru"),
                 ("bfloat16", "sgd", "lru"), ("float32", "sgd", "lfu"), ("float64", "sgd", "lru")):
        assert want in conf
    assert conf.count(("float32", "sgd", "lru")) >= 2


def test_universe():
    uni = L.universe(L.CASES[0].seed)
    assert 2300 <= uni.keys.size <= 2700 and np.unique(uni.keys).size == uni.keys.size
    for k in (-1, 0, L.I64MIN, L.I64MAX):
        assert k in uni.keys.tolist()
    assert (uni.keys < 0).sum() > 500 and (uni.keys > 0).sum() > 500
    for i, g in enumerate(uni.groups):
        assert 30 <= g.size <= 40
        for slots in (2048, 4096, 8192):        # one home line at every size of the walk
            lines = np.unique(L.home_line(g, slots))
            assert lines.size == 1
            if i == 0:
                assert lines[0] == slots // 8 - 1       # the last line
    assert np.isin(uni.sample[:56], uni.keys).all() and not np.isin(uni.sample[56:], uni.keys).any()


def test_the_walk_is_a_pure_function_of_the_case():
    a, b = L.generate(L.CASES[0]), L.generate(L.CASES[0])
    assert [L.describe(o) for o in a] == [L.describe(o) for o in b]
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for f in x:
            np.testing.assert_array_equal(x[f], y[f])
    assert [L.describe(o) for o in a] != [L.describe(o) for o in L.generate(L.CASES[-1])]


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_walk_is_not_vacuous(case):
    ops = L.generate(case)
    assert 150 <= len(ops) <= 170
    for op in ops:
        if "keys" in op:
            assert 1 <= op["keys"].size <= L.MAX_BATCH
    m, last_line, clustered = L.group_peaks(case, ops)
    s = m.stats
    # re-created after a removal, the three eviction routes together
    assert s["recreated"] >= 300
    assert min(s["evicted_remove"], s["evicted_budget"], s["evicted_shrink"]) >= 50
    assert s["evicted_sync"] >= 1
    # the EV under stress has to grow (1 024 rows at the start)
    assert m.creations > 4096 and m.peak >= 1500
    assert s["compacts_with_holes"] >= 5 and s["syncs"] >= 4 and s["marks_after_compact"] >= 3
    assert last_line >= 20 and clustered >= 20
    for k in (-1, 0):
        assert m.history[k].startswith("crc"), (k, m.history[k])
    names = {op["op"] for op in ops}
    assert names == {"insert", "upsert", "mark", "base", "lookup", "lookup_ro", "train", "remove",
                     "budget", "shrink", "compact", "reserve", "sync"}
    # duplicates where the API allows them, absent keys among the removed
    assert any(np.unique(o["keys"]).size < o["keys"].size for o in ops if o["op"] == "train")
    assert any(np.unique(o["keys"]).size < o["keys"].size for o in ops if o["op"] == "remove")
    for o in ops:
        if o["op"] in ("insert", "upsert"):
            assert np.unique(o["keys"]).size == o["keys"].size
    assert [o["gs"] for o in ops if o["op"] == "train"] == list(range(1, m.gs + 1))


@pytest.mark.parametrize("case", L.CASES[:2], ids=L.case_id)
def test_a_model_passes_its_own_walk(case):
    ops = L.generate(case)
    m = L.run_walk(case, ops, L.Model(case))
    assert m.rep is not None and len(m.rep) > 100


# ---------------------------------------------------------------------------
# The walk bites: planted lifecycle bugs, caught by the walk's own comparison
# ---------------------------------------------------------------------------
class KeepsTheMarkOfAnEvictedKey(L.Model):
    """The update bit stays with the KEY: it shows again when the key is re-created."""

    def _drop(self, k, route):
        was = k in self.marked
        super()._drop(k, route)
        if was:
            self.marked.add(k)


class KeepsTheVersionOfARecreatedKey(L.Model):
    """A re-created key finds the version its dead row had."""

    def __init__(self, case):
        super().__init__(case)
        self.old = {}

    def _drop(self, k, route):
        self.old[k] = self.rows[k].ver
        super()._drop(k, route)

    def _create(self, k, col, span):
        super()._create(k, col, span)
        self.rows[k].ver = self.old.get(k, 0)


@pytest.mark.parametrize("mutant,field", [(KeepsTheMarkOfAnEvictedKey, "updated"),
                                          (KeepsTheVersionOfARecreatedKey, "version")])
def test_a_planted_bug_is_caught_within_the_first_walk(mutant, field):
    case = L.CASES[0]
    ops = L.generate(case)
    with pytest.raises(AssertionError) as e:
        L.run_walk(case, ops, mutant(case))
    msg = str(e.value)
    assert "seed %d" % case.seed in msg and "failed at operation #" in msg
    assert msg.count("\n  #") == 10                     # the last ten operations
    assert field in msg.splitlines()[-1] and "the model" in msg.splitlines()[-1]
