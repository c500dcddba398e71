"""CPU: the walks tests/test_gpu_host_tier_incr.py replays are not vacuous.
For every seed the GPU test uses, the dict model alone (tests/
host_tier_incr_walk.py) must see each event the feature is about at least
NEED times, the table grow while the tier holds marked keys, and every kind of
operation happen; the generator is a pure function of its case."""
import numpy as np
import pytest

import host_tier_incr_walk as W


@pytest.fixture(scope="module", params=W.CASES, ids=W.case_id)
def walk(request):
    case = request.param
    ops = W.generate(case)
    return case, ops, W.replay(case, ops)


def test_each_event_happens_often_enough(walk):
    case, ops, m = walk
    for name in W.EVENTS:
        assert m.stats[name] >= W.NEED, (W.case_id(case), name, dict(m.stats))
    assert m.stats["tier_marked"] >= W.NEED         # public mark_updated reached the tier
    assert m.stats["clears"] >= 3


def test_the_table_grows_while_the_tier_holds_marked_keys(walk):
    case, ops, m = walk
    assert m.peak_top_flagged > W.MIN_ROWS, m.peak_top_flagged


def test_every_operation_kind_happens(walk):
    case, ops, m = walk
    names = [o["op"] for o in ops]
    for name in ("train", "lookup", "demote", "remove", "shrink", "mark", "clear", "track_off",
                 "track_on"):
        assert name in names, name
    assert W.N_OPS <= len(ops) <= W.N_OPS + 1
    dem = [o for o in ops if o["op"] == "demote"]
    assert {o["compact"] for o in dem} == {True, False}
    assert min(o["n"] for o in dem) >= W.BUDGETS[0] and max(o["n"] for o in dem) <= W.BUDGETS[1]
    off = names.index("track_off")
    on = names.index("track_on", off)
    assert on > off + 1                             # operations ran while tracking was off
    assert m.tracking and len(m.tier) > 0
    # live rows span several 32-bit bitmap words, the special keys are in play
    assert len(m.hbm) > 4 * 32
    seen = np.unique(np.concatenate([o["keys"] for o in ops if "keys" in o]))
    assert np.isin(W.universe(case.seed)[0][:4], seen).all()


def test_the_generator_is_a_pure_function_of_its_case(walk):
    case, ops, m = walk
    again = W.generate(case)
    assert len(again) == len(ops)
    for a, b in zip(ops, again):
        assert a["op"] == b["op"]
        if "keys" in a:
            assert np.array_equal(a["keys"], b["keys"])
    o1, o2 = m.observe(), W.replay(case, again).observe()
    for name in o1:
        assert np.array_equal(o1[name], o2[name]), name


def test_cases_cover_the_parametrisations():
    assert len(W.CASES) == 3
    assert any(c.by_row for c in W.CASES)
    assert any(c.policy == "lfu" and c.filter_freq for c in W.CASES)
    assert any(c.opt == "adagrad" for c in W.CASES) and any(c.opt == "sgd" for c in W.CASES)
