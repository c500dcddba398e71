"""The key budget at save time (KeyBudgetEvict through checkpoint.save and
checkpoint.save_incremental), end to end.

The reference is numpy on the trainer's export() taken just before the save:
    m = where(version == -1, INT64_MAX, version)
    victims = keys[np.lexsort((keys, m))[:N - max_keys]]
Keys are non-negative throughout: a save drops negative keys.
"""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 16
BUDGET = 300
I64MAX = np.iinfo(np.int64).max


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _snap(ev):
    k, v, ve, fr = ev.export()
    return (k.cpu().numpy(), v.cpu().numpy().view(np.uint32), ve.cpu().numpy(), fr.cpu().numpy())


def _train(dr, ev, opt, keys, gs, rng):
    ev.sparse_read(_t(keys))                                     # the training path creates
    ev.pending_grads.append(dr.IndexedSlices(
        _t(rng.standard_normal((keys.size, D)).astype(np.float32)), _t(keys)))
    opt.apply_gradients([ev], global_step=gs)
    assert not ev.pending_grads


def _kept(snap, max_keys):
    """The reference: the snapshot's keys that the budget keeps, ascending."""
    k, ve = snap[0], snap[2]
    m = np.where(ve == -1, I64MAX, ve)
    E = max(k.size - max_keys, 0)
    return np.sort(k[np.lexsort((k, m))[E:]])


def _budget_ev(dr, name):
    opt = dr.EmbeddingVariableOption(evict_option=dr.KeyBudgetEvict(
        max_keys=BUDGET, policy="lru", steps_to_live=10**9))
    ev = dr.EmbeddingVariable(name, D, 0.05, ev_option=opt, capacity=2048, device=DEV)
    assert (ev.max_keys, ev.policy, ev.steps_to_live) == (BUDGET, "lru", 10**9)
    return ev


def test_full_save_keeps_the_budget_and_restores(tmp_path):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    rng = np.random.default_rng(41)
    keys = rng.permutation(np.arange(0, 3000, 3, dtype=np.int64))       # 1 000 keys
    ev = _budget_ev(dr, "bgck_full")
    opt = dr.GradientDescentOptimizer(0.05)
    _train(dr, ev, opt, keys, 10, rng)
    _train(dr, ev, opt, keys[:600], 20, rng)
    _train(dr, ev, opt, keys[:150], 30, rng)
    before = _snap(ev)
    assert before[0].size == 1000 and sorted(set(before[2].tolist())) == [10, 20, 30]
    kept = _kept(before, BUDGET)
    # the 150 keys of step 30 and the 150 LARGEST keys of step 20: ties go by ascending key
    assert kept.size == BUDGET and np.isin(keys[:150], kept).all()
    assert np.isin(np.sort(keys[150:600])[-150:], kept).all()
    prefix = ck.save(str(tmp_path / "full"), {"emb": ev}, global_step=30, compact=True)
    assert ev.rows_allocated() == BUDGET == int(ev.total_count()[0])
    after = _snap(ev)
    sel = np.isin(before[0], kept)
    assert before[3].size == 0 == after[3].size                          # no filter: no freqs
    for a, b in zip(after[:3], before[:3]):
        np.testing.assert_array_equal(a, b[sel])
    fresh = dr.EmbeddingVariable("bgck_full_restored", D, 0.05, steps_to_live=10**9,
                                 capacity=2048, device=DEV)
    ck.restore(prefix, {"emb": fresh})
    got = _snap(fresh)
    np.testing.assert_array_equal(got[0], kept)
    np.testing.assert_array_equal(got[1], before[1][sel])               # rows bit-equal
    np.testing.assert_array_equal(got[2], before[2][sel])
    assert fresh.rows_allocated() == BUDGET
    dr.status_check()


def test_replica_fed_by_deltas_stays_inside_the_budget(tmp_path):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    rng = np.random.default_rng(42)
    ev = _budget_ev(dr, "bgck_delta_trainer")
    opt = dr.GradientDescentOptimizer(0.05)
    _train(dr, ev, opt, np.arange(0, 250, dtype=np.int64), 1, rng)
    full = ck.save(str(tmp_path / "base"), {"emb": ev}, global_step=1)
    assert int(ev.total_count()[0]) == 250                      # the budget does not bite yet
    rep = dr.EmbeddingVariable("bgck_delta_replica", D, 0.05, steps_to_live=10**9,
                               capacity=2048, device=DEV)
    ck.restore(full, {"emb": rep})
    ev.track_updates()
    ev.track_removals()
    rounds = [
        (10, np.concatenate([np.arange(0, 50), np.arange(250, 450)]).astype(np.int64), None),
        (20, np.concatenate([np.arange(200, 250), np.arange(1000, 1100)]).astype(np.int64), 20),
    ]
    for gs, touched, save_gs in rounds:
        _train(dr, ev, opt, touched, gs, rng)
        before = _snap(ev)
        assert before[0].size > BUDGET
        kept = _kept(before, BUDGET)
        # with and without global_step: the budget is applied either way
        delta = ck.save_incremental(str(tmp_path / ("delta_%d" % gs)), {"emb": ev},
                                    global_step=save_gs)
        r = ck.BundleReader(delta)
        np.testing.assert_array_equal(np.sort(r.lookup("emb-sparse_incr_removed_keys")),
                                      np.setdiff1d(before[0], kept))
        ts = _snap(ev)
        np.testing.assert_array_equal(ts[0], kept)
        assert ev.rows_allocated() == before[0].size           # save_incremental does not compact
        ck.restore_incremental(delta, {"emb": rep}, compact=True)
        rs = _snap(rep)
        for a, b in zip(rs, ts):
            np.testing.assert_array_equal(a, b)                 # same keys, rows bit for bit
        assert rep.rows_allocated() == BUDGET <= ev.max_keys
        ev.compact()
    dr.status_check()


def _files(prefix):
    out = {}
    for p in sorted(glob.glob(prefix + "*")):
        with open(p, "rb") as f:
            out[os.path.basename(p)[len(os.path.basename(prefix)):]] = f.read()
    assert out
    return out


def test_no_budget_saves_what_it_saved_before(tmp_path):
    """max_keys = 0 is off: the bundles of an EV built with KeyBudgetEvict(0)
    and of its twin built with GlobalStepEvict are byte-identical, full save
    and delta."""
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    rng = np.random.default_rng(43)
    keys = rng.permutation(np.arange(0, 1500, dtype=np.int64))[:800]
    vals = rng.standard_normal((800, D)).astype(np.float32)
    vers = rng.integers(0, 9, 800).astype(np.int64)
    evs = []
    for i, eo in enumerate((dr.KeyBudgetEvict(max_keys=0, steps_to_live=4),
                            dr.GlobalStepEvict(steps_to_live=4))):
        ev = dr.EmbeddingVariable("bgck_off_%d" % i, D, 0.05, capacity=2048, device=DEV,
                                  ev_option=dr.EmbeddingVariableOption(evict_option=eo))
        assert ev.max_keys == 0 and ev.steps_to_live == 4
        ev.insert(_t(keys), _t(vals), _t(vers))
        ev.track_updates()
        ev.track_removals()
        ev.mark_updated(_t(keys[::3]))
        evs.append(ev)
    full = [_files(ck.save(str(tmp_path / ("full_%d" % i)), {"emb": ev}, global_step=9,
                           compact=True)) for i, ev in enumerate(evs)]
    assert full[0] == full[1]
    assert 0 < int(evs[0].total_count()[0]) < 800               # the age rule did act
    delta = [_files(ck.save_incremental(str(tmp_path / ("delta_%d" % i)), {"emb": ev},
                                        global_step=11)) for i, ev in enumerate(evs)]
    assert delta[0] == delta[1]
    assert int(evs[0].total_count()[0]) == int(evs[1].total_count()[0])
    dr.status_check()
