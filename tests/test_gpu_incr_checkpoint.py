"""Incremental EV checkpoints end to end: a trainer's EVs track the keys its
optimizer updates, save_incremental writes them, restore_incremental applies
them to a replica that was restored from an earlier full save.  Afterwards the
replica's export() -- primaries and optimizer slots -- must equal the
trainer's bit for bit, and a read-only lookup must serve the same rows.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 16


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _snap(ev):
    k, v, ve, fr = ev.export()
    return (k.cpu().numpy(), v.cpu().numpy().view(np.uint32), ve.cpu().numpy(), fr.cpu().numpy())


def _same(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y)


def _multihot(rng, B, H, vocab):
    lens = rng.integers(1, H + 1, B)
    rows = np.repeat(np.arange(B), lens)
    cols = np.concatenate([np.arange(n) for n in lens])
    return (np.stack([rows, cols], 1).astype(np.int64),
            rng.integers(0, vocab, rows.shape[0]).astype(np.int64), (B, H))


BASE = np.concatenate([np.arange(600), np.arange(5000, 7000)]).astype(np.int64)
UNTOUCHED = np.arange(5000, 5200, dtype=np.int64)
ABSENT = np.arange(200, dtype=np.int64) + 10**9


def _batches(seed, steps=3, B=200, H=4):
    """Per step and table about 500 ids; the id range widens every step, so
    each step brings keys the tables have not seen."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(steps):
        sps = [_multihot(rng, B, H, 700 + 400 * s) for _ in range(2)]
        out.append((sps, rng.standard_normal((B, D)).astype(np.float32)))
    return out


def _tables(dr, tag, fill=True):
    rng = np.random.default_rng(11)
    evs = []
    for f in range(2):
        ev = dr.EmbeddingVariable("%s_%d" % (tag, f), D, 0.05 * (f + 1), device=DEV,
                                  capacity=1024)
        vals = rng.standard_normal((BASE.size, D)).astype(np.float32)
        if fill:
            ev.insert(_t(BASE), _t(vals))
        evs.append(ev)
    return evs


def _step(dr, evs, opt, batch, gs):
    sps, g = batch
    out = None
    for ev, (i, v, s) in zip(evs, sps):
        o = dr.embedding_lookup_sparse(ev, dr.SparseTensor(_t(i), _t(v), s), combiner="mean")
        out = o if out is None else out + o
    out.backward(_t(g))
    pend = [ev.pending_grads[-1] for ev in evs]
    opt.apply_gradients(evs, global_step=gs)
    assert all(not ev.pending_grads for ev in evs)
    return pend


def _named(evs, slot):
    d = {}
    for f, ev in enumerate(evs):
        d["emb%d" % f] = ev
        if slot:
            d["emb%d/Adagrad" % f] = ev.slot("Adagrad", 0.1)
    return d


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_delta_brings_a_replica_up_to_date(tmp_path, optimizer):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    slot = optimizer == "adagrad"
    opt = dr.AdagradOptimizer(0.05) if slot else dr.GradientDescentOptimizer(0.05)
    a = _tables(dr, "incr_e2e_a_" + optimizer)
    b = _tables(dr, "incr_e2e_b_" + optimizer, fill=False)
    va, vb = _named(a, slot), _named(b, slot)
    full = ck.save(str(tmp_path / "full"), va)
    ck.restore(full, vb)
    for n in va:
        _same(_snap(vb[n]), _snap(va[n]))
    for ev in a:
        ev.track_updates()
    batches = _batches(5)
    for s, batch in enumerate(batches):
        pend = _step(dr, a, opt, batch, s + 1)
        if not slot:    # SGD: a tracked group leaves the fused backward + update path
            assert not any(getattr(p, "_pending").applied for p in pend)
    touched = [np.unique(np.concatenate([bt[0][f][1] for bt in batches])) for f in range(2)]
    for f in range(2):
        assert a[f].updated_count() == touched[f].size
        assert not np.isin(touched[f], BASE).all()            # the steps created keys
    delta = ck.save_incremental(str(tmp_path / "delta"), va, global_step=3)
    r = ck.BundleReader(delta)
    for f in range(2):
        n_delta = r.dtype_and_shape("emb%d-sparse_incr_keys" % f)[1][0]
        assert n_delta == touched[f].size < a[f].total_count()[0].item()
        np.testing.assert_array_equal(np.sort(r.lookup("emb%d-sparse_incr_keys" % f)), touched[f])
    assert sorted(r.keys()) == sorted(n + "-sparse_incr_" + t for n in va for t in
                                      ("partition_offset", "keys", "values", "versions", "freqs"))
    before = [ev.total_count()[0].item() for ev in b]
    ck.restore_incremental(delta, vb)
    for n in va:
        _same(_snap(vb[n]), _snap(va[n]))
    assert all(ev.total_count()[0].item() > n0 for ev, n0 in zip(b, before))   # keys arrived
    with dr.read_only_lookups():
        for f in range(2):
            q = _t(np.concatenate([touched[f], UNTOUCHED, ABSENT]))
            ra, rb = a[f].sparse_read(q), b[f].sparse_read(q)
            np.testing.assert_array_equal(rb.cpu().numpy().view(np.uint32),
                                          ra.cpu().numpy().view(np.uint32))
    # the save cleared the marks: a second delta right after it is empty
    for f in range(2):
        assert a[f].updated_count() == 0
    again = ck.save_incremental(str(tmp_path / "delta2"), va)
    r2 = ck.BundleReader(again)
    for n in va:
        assert r2.dtype_and_shape(n + "-sparse_incr_keys")[1] == (0,)
        assert r2.dtype_and_shape(n + "-sparse_incr_values")[1] == (0, D)
    dr.status_check()


def test_sgd_values_do_not_depend_on_tracking():
    """With tracking off SGD runs the backward fused with the update; with it
    on the gradient is formed and applied the ordinary way.  Same tables."""
    import deeprec_amd as dr
    batches = _batches(6)
    snaps = {}
    for on in (False, True):
        evs = _tables(dr, "incr_sgd_%d" % on)
        if on:
            for ev in evs:
                ev.track_updates()
        opt = dr.GradientDescentOptimizer(0.05)
        for s, batch in enumerate(batches):
            pend = _step(dr, evs, opt, batch, s + 1)
            assert all(p._pending.applied for p in pend) == (not on)
        if on:
            assert all(ev.updated_count() > 0 for ev in evs)
        snaps[on] = [_snap(ev) for ev in evs]
    for x, y in zip(snaps[False], snaps[True]):
        _same(x, y)
    dr.status_check()


@pytest.mark.parametrize("partition_num", [1, 3])
def test_delta_restores_onto_another_partition_count(tmp_path, partition_num):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    rng = np.random.default_rng(40 + partition_num)
    allk = np.unique(np.concatenate([np.arange(-40, 0), rng.integers(0, 200000, 4200)])
                     ).astype(np.int64)
    rng.shuffle(allk)
    src, marked = [], []
    for p in range(2):
        keys = allk[p::2]
        keys = np.concatenate([keys[keys < 0], keys[keys >= 0]])   # the negatives get marked
        ev = dr.EmbeddingVariable("incr_rp_src_%d_%d" % (partition_num, p), 8, 0.5, device=DEV,
                                  capacity=1024, steps_to_live=3)
        ev.insert(_t(keys), _t(rng.standard_normal((keys.size, 8)).astype(np.float32)),
                  _t(rng.integers(0, 100, keys.size).astype(np.int64)))
        ev.track_updates()
        mk = keys[:keys.size // 3]
        ev.mark_updated(_t(mk))
        src.append(ev)
        marked.append(mk)
    snaps = [_snap(ev) for ev in src]
    k = np.concatenate([s[0] for s in snaps])
    v = np.concatenate([s[1] for s in snaps])
    ve = np.concatenate([s[2] for s in snaps])
    in_delta = np.isin(k, np.concatenate(marked)) & (k >= 0)      # negative keys are not saved
    assert (np.concatenate(marked) < 0).any()
    pre = ck.save_incremental(str(tmp_path / "d"),
                              {"scope/emb/part_%d/x" % p: src[p] for p in range(2)})
    stale = k[in_delta][::7]                                       # rows the delta must overwrite
    landed = 0
    for pid in range(partition_num):
        ev = dr.EmbeddingVariable("incr_rp_dst_%d_%d" % (partition_num, pid), 8, 0.5, device=DEV,
                                  capacity=1024, steps_to_live=3)
        mine = stale[stale % 1000 % partition_num == pid]
        ev.insert(_t(mine), _t(np.full((mine.size, 8), 9.0, np.float32)),
                  _t(np.zeros(mine.size, np.int64)))
        ck.restore_incremental(pre, {"scope/emb/part_%d/x" % pid: ev}, pid, partition_num)
        sel = in_delta & (k % 1000 % partition_num == pid)         # (k >= 0 here: % is C's)
        o = np.argsort(k[sel])
        gk, gv, gve, _ = _snap(ev)
        np.testing.assert_array_equal(gk, k[sel][o])
        np.testing.assert_array_equal(gv, v[sel][o])
        np.testing.assert_array_equal(gve, ve[sel][o])
        assert (gk % 1000 % partition_num == pid).all()
        landed += gk.size
    assert landed == in_delta.sum() > 0
