"""Incremental EV checkpoints that carry evictions, end to end.

A trainer EV (64 fp32 columns, an Adagrad slot, steps_to_live 2) tracks its
updates and logs its removals.  A replica restores a full save and is then fed
by deltas alone: save_incremental(global_step) shrinks the trainer, writes the
updated rows and the removed keys; restore_incremental(compact=True) removes,
upserts and compacts.  Afterwards the replica holds exactly the trainer's keys
(without the keys that were evicted, re-created by a lookup and never updated:
both sides serve the default for those), bit for bit in both columns, and its
row count equals its key count.

Timeline (global step 2 * s for training step s; a key goes when
global_step - version > 2):
  A  updated at every step                      -> always kept
  B  never seen after the base                  -> evicted by delta 1
  C  evicted by delta 1, updated at steps 3, 4  -> back, with the new row
  D  evicted by delta 1, looked up at step 3    -> absent on the replica
  E  updated at steps 1, 2 only                 -> evicted by delta 2
  F  created at step 2, updated at 2, 3, 4      -> arrives by delta 1
  G  created and updated at step 1 only         -> arrives by delta 1, evicted by delta 2
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64

A = np.concatenate([np.arange(0, 800), [-1, -7]]).astype(np.int64)
B = np.concatenate([np.arange(800, 1100), [-3]]).astype(np.int64)
C_ = np.arange(1100, 1200, dtype=np.int64)
D_ = np.arange(1200, 1300, dtype=np.int64)
E = np.arange(1300, 2000, dtype=np.int64)
F = np.arange(5000, 5200, dtype=np.int64)
G = np.arange(6000, 6100, dtype=np.int64)
BASE = np.concatenate([A, B, C_, D_, E])
STEPS = [np.concatenate([A, E, G]), np.concatenate([A, E, F]),
         np.concatenate([A, C_, F]), np.concatenate([A, C_, F])]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _snap(ev):
    k, v, ve, fr = ev.export()
    return (k.cpu().numpy(), v.cpu().numpy().view(np.uint32), ve.cpu().numpy(), fr.cpu().numpy())


def _only(snap, keep):
    return tuple(a[keep] if a.shape[0] == keep.size else a for a in snap)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (x.shape, y.shape)
        np.testing.assert_array_equal(x, y)


def _ev(dr, name):
    ev = dr.EmbeddingVariable(name, D, 0.05, steps_to_live=2, capacity=4096, device=DEV)
    return ev, ev.slot("Adagrad", 0.1)


def _train(dr, ev, opt, keys, gs, rng):
    ev.sparse_read(_t(keys))                                     # the training path creates
    ev.pending_grads.append(dr.IndexedSlices(
        _t(rng.standard_normal((keys.size, D)).astype(np.float32)), _t(keys)))
    opt.apply_gradients([ev], global_step=gs)
    assert not ev.pending_grads


class _Run(object):
    """The trainer's timeline with a set of replicas fed by its deltas."""

    def __init__(self, dr, ck, tmp_path, tag, tname, replicas, removals=True):
        self.dr, self.ck, self.dir, self.removals = dr, ck, tmp_path, removals
        rng = self.rng = np.random.default_rng(99)
        self.ev, self.acc = _ev(dr, tag + "_trainer")
        self.vars = {tname: self.ev, tname + "/Adagrad": self.acc}
        self.ev.insert(_t(BASE), _t(rng.standard_normal((BASE.size, D)).astype(np.float32)),
                       _t(np.zeros(BASE.size, np.int64)))
        self.acc.insert(_t(BASE), _t(rng.random((BASE.size, D)).astype(np.float32) + 0.1))
        self.opt = dr.AdagradOptimizer(0.05)
        full = ck.save(str(tmp_path / (tag + "_full")), self.vars, global_step=0)
        assert int(self.ev.total_count()[0]) == BASE.size        # nothing is old enough yet
        self.replicas = []
        for rname, pid, pnum in replicas:
            ev, acc = _ev(dr, "%s_replica_%d" % (tag, pid))
            rv = {rname: ev, rname + "/Adagrad": acc}
            ck.restore(full, rv, pid, pnum)
            self.replicas.append((ev, acc, rv, pid, pnum))
        self.ev.track_updates()
        if removals:
            self.ev.track_removals()
        self.deltas = []

    def steps(self, first, last):
        for s in range(first, last + 1):
            _train(self.dr, self.ev, self.opt, STEPS[s - 1], 2 * s, self.rng)
            if s == 3:
                self.ev.sparse_read(_t(D_))                      # re-created, never updated

    def delta(self, gs):
        p = self.ck.save_incremental(str(self.dir / ("delta_%d" % gs)), self.vars, global_step=gs)
        self.deltas.append(p)
        for ev, acc, rv, pid, pnum in self.replicas:
            self.ck.restore_incremental(p, rv, pid, pnum, compact=self.removals)
        return p


def test_replica_fed_by_deltas_converges_and_stays_bounded(tmp_path):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    run = _Run(dr, ck, tmp_path, "incr_ev", "emb", [("emb", 0, 1)])
    rev, racc = run.replicas[0][:2]
    nonneg = BASE[BASE >= 0]
    np.testing.assert_array_equal(_snap(rev)[0], np.sort(nonneg))

    run.steps(1, 2)
    d1 = run.delta(4)
    r = ck.BundleReader(d1)
    gone1 = np.concatenate([B, C_, D_])
    np.testing.assert_array_equal(np.sort(r.lookup("emb-sparse_incr_removed_keys")),
                                  np.sort(gone1[gone1 >= 0]))
    offs = r.lookup("emb-sparse_incr_removed_partition_offset")
    assert offs.dtype == np.int32 and offs.shape == (1001,) and offs[-1] == (gone1 >= 0).sum()
    assert not r.contains("emb/Adagrad-sparse_incr_removed_keys")
    assert run.ev.removed_count() == 0 and run.ev.updated_count() == 0   # cleared by the save
    # no key has been re-created yet: the replica IS the trainer (its non-negative keys)
    for t, rp in ((run.ev, rev), (run.acc, racc)):
        ts = _snap(t)
        _same(_snap(rp), _only(ts, ts[0] >= 0))
    assert not np.isin(gone1, _snap(rev)[0]).any()
    assert rev.rows_allocated() == int(rev.total_count()[0])

    run.steps(3, 4)
    run.delta(8)
    tk = _snap(run.ev)[0]
    assert not np.isin(np.concatenate([B, E, G]), tk).any() and np.isin(C_, tk).all()
    for t, rp in ((run.ev, rev), (run.acc, racc)):
        ts, rs = _snap(t), _snap(rp)
        # every key the trainer has updated or kept since the base, bit for bit; D was
        # evicted, re-created by a lookup and never updated: the replica serves the default
        _same(rs, _only(ts, (ts[0] >= 0) & ~np.isin(ts[0], D_)))
    rk = _snap(rev)[0]
    np.testing.assert_array_equal(rk, np.sort(np.concatenate([A[A >= 0], C_, F])))
    for name, grp in (("B", B), ("D", D_), ("E", E), ("G", G)):
        assert not np.isin(grp, rk).any(), name                  # today's code keeps them all
    # C carries the trainer's NEW row (version 8), not the base row it had before its eviction
    k, _, ve, _ = _snap(rev)
    assert (ve[np.isin(k, C_)] == 8).all()
    assert rev.rows_allocated() == int(rev.total_count()[0]) == rk.size
    with dr.read_only_lookups():
        q = _t(np.concatenate([C_, D_, E[:50], A[:50]]))
        np.testing.assert_array_equal(rev.sparse_read(q).cpu().numpy().view(np.uint32),
                                      run.ev.sparse_read(q).cpu().numpy().view(np.uint32))
    dr.status_check()


FIVE = ("partition_offset", "keys", "values", "versions", "freqs")


def test_delta_without_removal_tracking_is_todays(tmp_path):
    """Tracking off: exactly the five tensors per name, and the delta applies
    through restore_incremental as before -- updated rows land, the keys the
    trainer evicted stay on the replica until its next full restore."""
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    run = _Run(dr, ck, tmp_path, "incr_ev_off", "emb", [("emb", 0, 1)], removals=False)
    rev, racc = run.replicas[0][:2]
    base = [_snap(rev), _snap(racc)]
    run.steps(1, 2)
    d1 = run.delta(4)
    assert sorted(ck.BundleReader(d1).keys()) == sorted(
        n + "-sparse_incr_" + t for n in run.vars for t in FIVE)
    gone = np.concatenate([B, C_, D_])
    gone = gone[gone >= 0]
    for t, rp, b in ((run.ev, rev, base[0]), (run.acc, racc, base[1])):
        ts, rs = _snap(t), _snap(rp)
        assert not np.isin(gone, ts[0]).any()                    # the trainer shrank
        _same(_only(rs, ~np.isin(rs[0], gone)), _only(ts, ts[0] >= 0))
        _same(_only(rs, np.isin(rs[0], gone)), _only(b, np.isin(b[0], gone)))
    assert rev.rows_allocated() == int(rev.total_count()[0])     # no hole was made
    dr.status_check()


def test_two_partition_replicas_split_the_trainers_keys(tmp_path):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    run = _Run(dr, ck, tmp_path, "incr_ev_part", "emb/part_0",
               [("emb/part_0", 0, 2), ("emb/part_1", 1, 2)])
    run.steps(1, 2)
    run.delta(4)
    run.steps(3, 4)
    run.delta(8)
    ts = _snap(run.ev)
    want = (ts[0] >= 0) & ~np.isin(ts[0], D_)
    got = []
    for ev, acc, rv, pid, pnum in run.replicas:
        rs = _snap(ev)
        assert (rs[0] % 1000 % 2 == pid).all() and rs[0].size > 200
        _same(rs, _only(ts, want & (ts[0] % 1000 % 2 == pid)))
        assert ev.rows_allocated() == int(ev.total_count()[0])
        got.append(rs[0])
    assert np.intersect1d(got[0], got[1]).size == 0
    np.testing.assert_array_equal(np.sort(np.concatenate(got)), ts[0][want])
    dr.status_check()
