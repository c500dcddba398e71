"""Update tracking by row (dr_ev_mark_updated_rows, track_updates(by_row=True)):
the mark takes the rows a lookup resolved instead of probing the key table
again.  It must set exactly the bits the mark by key sets -- compared through
updated_count() and export_updated() against twin tables marked by key -- in
both row layouts of the row-grouped backward, and a tracked SGD group must
keep the fused backward + update.
"""
import ctypes as C

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


def _upd(ev):
    k, v, ve, fr = ev.export_updated()
    return (k.cpu().numpy(), v.cpu().numpy().view(np.uint32), ve.cpu().numpy(), fr.cpu().numpy())


def _same(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y)


def _same_marks(a, b):
    assert a.updated_count() == b.updated_count()
    _same(_upd(a), _upd(b))


def _row_capacity(dr, ev):
    return dr._lib.lib().dr_ev_row_capacity(ev.handle)


def _table(dr, name, keys, seed, **kw):
    """An EV holding `keys`; twins built with the same arguments hold the same
    keys and values (not necessarily in the same rows)."""
    ev = dr.EmbeddingVariable(name, D, 0.05, device=DEV, capacity=1024, **kw)
    vals = np.random.default_rng(seed).standard_normal((keys.size, D)).astype(np.float32)
    ev.insert(_t(keys), _t(vals))
    return ev


def _c_mark_rows(dr, evs, rows, rows_record=0, koff=None):
    """The C entry itself (the Python wrappers leave out empty and untracked
    tables): evs[t] an EV or None, rows[t] its device rows."""
    from deeprec_amd._lib import check, lib, ptr, stream_handle
    T = len(evs)
    if koff is None:
        koff = [0]
        for r in rows:
            koff.append(koff[-1] + r.numel())
        flat = torch.cat([r.reshape(-1) for r in rows]).contiguous()
    else:
        flat = rows
    handles = (C.c_void_p * T)(*[None if e is None else e.handle.value for e in evs])
    check(lib().dr_ev_mark_updated_rows(handles, T, ptr(flat), (C.c_int64 * (T + 1))(*koff),
                                        rows_record, None, stream_handle(torch.device(DEV))))


KEYS = np.concatenate([[-1], np.arange(2500), np.arange(10**6, 10**6 + 500)]).astype(np.int64)
ABSENT = np.arange(10**9, 10**9 + 40, dtype=np.int64)


# -- 1 -------------------------------------------------------------------------
def test_row_mark_equals_key_mark():
    import deeprec_amd as dr
    a = _table(dr, "rowmark_eq_a", KEYS, 3)
    b = _table(dr, "rowmark_eq_b", KEYS, 3)
    a.track_updates()
    b.track_updates()
    rng = np.random.default_rng(17)
    pick = rng.choice(KEYS, 700)                                    # with repeats
    keys = np.concatenate([pick, ABSENT, [-1, -1], pick[:50]]).astype(np.int64)
    rng.shuffle(keys)
    assert np.unique(keys).size < keys.size
    present = np.unique(keys[np.isin(keys, KEYS)])
    a.mark_updated(_t(keys))
    rows = b.find(_t(keys))
    assert (rows.cpu().numpy() < 0).sum() == ABSENT.size           # the absent keys have no row
    b.mark_updated_rows(rows)
    assert b.updated_count() == present.size
    np.testing.assert_array_equal(_upd(b)[0], present)
    _same_marks(a, b)
    # rows out of range change nothing
    before = _upd(b)
    b.mark_updated_rows(_t(np.array([_row_capacity(dr, b) + 5, 2**40], np.int64)))
    assert b.updated_count() == present.size
    _same(_upd(b), before)
    # num_valid: only the first positions
    a.clear_updated()
    b.clear_updated()
    nv = _t(np.array([37], np.int64))
    a.mark_updated(_t(keys), nv)
    b.mark_updated_rows(rows, nv)
    first = np.unique(keys[:37][np.isin(keys[:37], KEYS)])
    assert 0 < first.size < present.size
    assert b.updated_count() == first.size
    np.testing.assert_array_equal(_upd(b)[0], first)
    _same_marks(a, b)
    dr.status_check()


# -- 2 -------------------------------------------------------------------------
def _triples(dr, tag):
    sets = [np.arange(100 * t, 100 * t + 1500 + 300 * t, dtype=np.int64) for t in range(3)]
    out = []
    for side in "ab":
        evs = [_table(dr, "rowmark_%s_%s%d" % (tag, side, t), sets[t], 20 + t) for t in range(3)]
        for ev in evs:
            ev.track_updates()
        out.append(evs)
    return sets, out[0], out[1]


def _draw(rng, keyset, n):
    """n keys of the table, repeats included, and a few it does not hold."""
    k = rng.choice(keyset, n).astype(np.int64)
    k[4::9] = np.resize(ABSENT, k[4::9].size)
    return k


def test_layouts_and_tails():
    import deeprec_amd as dr
    sets, a, b = _triples(dr, "lay")
    rng = np.random.default_rng(23)

    def clear():
        for ev in a + b:
            if ev.tracking_updates():
                ev.clear_updated()

    def run(sizes, evs_b=None, rows_record=0):
        keys = [_draw(rng, sets[t], n) for t, n in enumerate(sizes)]
        for t in range(len(sizes)):
            if keys[t].size:
                a[t].mark_updated(_t(keys[t]))
        rows = [b[t].find(_t(keys[t])) if keys[t].size
                else torch.empty(0, dtype=torch.int64, device=DEV) for t in range(len(sizes))]
        evs_b = b[:len(sizes)] if evs_b is None else evs_b
        if rows_record:
            B, T = sizes[0], len(sizes)
            block = torch.stack(rows, 1).contiguous().view(-1)          # [B, T] record-major
            _c_mark_rows(dr, evs_b, block, 1, [t * B for t in range(T + 1)])
        else:
            _c_mark_rows(dr, evs_b, rows)

    # position order, T = 3 (not a power of two), an empty table, block and wave tails
    run([257, 0, 65])
    for t in range(3):
        _same_marks(a[t], b[t])
    assert b[1].updated_count() == 0 and b[0].updated_count() > 0 and b[2].updated_count() > 0
    # one table: below, at and past a wave, and past several blocks
    for n in (1, 63, 64, 65, 2049):
        clear()
        run([n])
        _same_marks(a[0], b[0])
        assert 0 < b[0].updated_count() <= n
    # one of three tables not tracking
    clear()
    a[1].track_updates(False)
    b[1].track_updates(False)
    run([130, 70, 33])
    _same_marks(a[0], b[0])
    _same_marks(a[2], b[2])
    assert b[0].updated_count() > 0 and b[2].updated_count() > 0
    a[1].track_updates()
    b[1].track_updates()
    assert b[1].updated_count() == 0
    # one of three tables null: its key space stays unmarked
    clear()
    run([130, 70, 33], evs_b=[b[0], None, b[2]])
    _same_marks(a[0], b[0])
    _same_marks(a[2], b[2])
    assert a[1].updated_count() > 0 and b[1].updated_count() == 0
    # record-major [batch, T] rows, batch = 67, T = 3
    clear()
    run([67, 67, 67], rows_record=1)
    for t in range(3):
        _same_marks(a[t], b[t])
        assert b[t].updated_count() > 0
    # ... and with a null table in it
    clear()
    run([67, 67, 67], evs_b=[None, b[1], b[2]], rows_record=1)
    _same_marks(a[1], b[1])
    _same_marks(a[2], b[2])
    assert b[0].updated_count() == 0
    dr.status_check()


# -- 3 -------------------------------------------------------------------------
def test_rows_sharing_a_bitmap_word():
    import deeprec_amd as dr
    keys = np.arange(7, 7 + 2000, dtype=np.int64)
    ev = _table(dr, "rowmark_word", keys, 31)
    ev.track_updates()
    rows = ev.find(_t(keys)).cpu().numpy()
    n = ev.rows_allocated()
    assert n == keys.size and np.array_equal(np.sort(rows), np.arange(n))
    key_of = np.empty(n, np.int64)
    key_of[rows] = keys

    def check(marked_rows, distinct):
        ev.clear_updated()
        ev.mark_updated_rows(_t(np.asarray(marked_rows, np.int64)))
        assert ev.updated_count() == len(distinct)
        np.testing.assert_array_equal(_upd(ev)[0], np.sort(key_of[np.asarray(distinct)]))

    word = np.arange(64, 96)
    check(word, word)                                  # all 32 bits of one word from one wave
    check(np.concatenate([word, word[::-1]]), word)    # ... each of them twice, one wave
    check(np.full(256, 70), [70])                      # one row from every lane of a block
    check([n - 1], [n - 1])                            # the last allocated row
    check([n - 1, -3, 0], [n - 1, 0])                  # ... beside a default (negative) row
    dr.status_check()


# -- training flows --------------------------------------------------------------
def _multihot(rng, B, H, vocab):
    lens = rng.integers(1, H + 1, B)
    rows = np.repeat(np.arange(B), lens)
    cols = np.concatenate([np.arange(n) for n in lens])
    return (np.stack([rows, cols], 1).astype(np.int64),
            rng.integers(0, vocab, rows.shape[0]).astype(np.int64), (B, H))


BASE = np.arange(900, dtype=np.int64)


def _batches(seed, steps=3, B=300, H=6):
    """Per step and table about 1000 ids from a range that widens every step:
    each step creates keys, and the tables (row capacity 1024 at first) grow
    in the forward of more than one step."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(steps):
        sps = [_multihot(rng, B, H, 2500 * (s + 1)) for _ in range(2)]
        out.append((sps, rng.standard_normal((B, D)).astype(np.float32)))
    return out


def _tables(dr, tag, **kw):
    return [_table(dr, "%s_%d" % (tag, f), BASE, 11 + f, **kw) for f in range(2)]


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


def _touched(batches, f):
    return np.unique(np.concatenate([bt[0][f][1] for bt in batches]))


# -- 4 -------------------------------------------------------------------------
def test_tracked_sgd_keeps_the_fused_step():
    import deeprec_amd as dr
    batches = _batches(6)
    snaps = {}
    for on in (False, True):
        evs = _tables(dr, "rowmark_sgd_%d" % on)
        if on:
            for ev in evs:
                ev.track_updates(by_row=True)
                assert ev.tracking_updates() and ev.tracking_by_row()
        opt = dr.GradientDescentOptimizer(0.05)
        caps = []
        for s, batch in enumerate(batches):
            pend = _step(dr, evs, opt, batch, s + 1)
            assert all(p._pending.applied for p in pend)       # fused, tracked or not
            caps.append(_row_capacity(dr, evs[0]))
        assert caps[-1] > caps[0] > 1024          # the bitmap was regrown with bits in it
        if on:
            for f, ev in enumerate(evs):
                touched = _touched(batches, f)
                assert not np.isin(touched, BASE).all()        # the steps created keys
                assert ev.updated_count() == touched.size
                np.testing.assert_array_equal(_upd(ev)[0], touched)
        snaps[on] = [_snap(ev) for ev in evs]
    for x, y in zip(snaps[False], snaps[True]):
        _same(x, y)
    dr.status_check()


# -- 5 -------------------------------------------------------------------------
def _onehot_step(dr, evs, ids, g, opt, var_list, gs=None):
    B = ids.shape[0]
    ind = _t(np.stack([np.arange(B), np.zeros(B, np.int64)], 1).astype(np.int64))
    sps = [dr.SparseTensor(ind, _t(ids[:, t]), (B, 1)) for t in range(len(evs))]
    out = dr.embedding_lookup_sparse_multi(evs, sps, combiner="sum")
    out.backward(_t(g))
    pend = [ev.pending_grads[-1] for ev in evs]
    opt.apply_gradients(var_list, global_step=gs)
    return pend


def _onehot_batches(seed, T, steps=3, B=200):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(steps):
        ids = rng.integers(0, 150 + 1200 * s, (B, T)).astype(np.int64)   # repeats; new keys
        ids[1::5] = ids[0::5][:ids[1::5].shape[0]]
        out.append((ids, rng.standard_normal((B, T * D)).astype(np.float32)))
    return out


def test_onehot_group_record_major_rows():
    import deeprec_amd as dr
    T = 3
    batches = _onehot_batches(8, T)
    snaps = {}
    for on in (False, True):
        evs = [_table(dr, "rowmark_oh_%d_%d" % (on, t), BASE, 40 + t) for t in range(T)]
        if on:
            for ev in evs:
                ev.track_updates(by_row=True)
        opt = dr.GradientDescentOptimizer(0.05)
        for ids, g in batches:
            pend = _onehot_step(dr, evs, ids, g, opt, evs)
            assert len({id(p._pending) for p in pend}) == 1    # one group of three tables
            assert pend[0]._pending.group.rows_record          # the record-major branch runs
            assert all(p._pending.applied for p in pend)
        if on:
            for t, ev in enumerate(evs):
                touched = np.unique(np.concatenate([ids[:, t] for ids, _ in batches]))
                assert not np.isin(touched, BASE).all()
                assert ev.updated_count() == touched.size
                np.testing.assert_array_equal(_upd(ev)[0], touched)
        snaps[on] = [_snap(ev) for ev in evs]
    for x, y in zip(snaps[False], snaps[True]):
        _same(x, y)
    dr.status_check()


def test_onehot_group_partly_in_var_list():
    import deeprec_amd as dr
    T = 3
    (ids, g), = _onehot_batches(9, T, steps=1)
    evs = [_table(dr, "rowmark_part_%d" % t, BASE, 50 + t) for t in range(T)]
    for ev in evs:
        ev.track_updates(by_row=True)
    opt = dr.GradientDescentOptimizer(0.05)
    pend = _onehot_step(dr, evs, ids, g, opt, [evs[0], evs[2]])
    assert pend[0]._pending.group.rows_record
    assert not pend[0]._pending.applied            # a group partly in var_list is not fused
    for t in (0, 2):
        touched = np.unique(ids[:, t])
        assert evs[t].updated_count() == touched.size
        np.testing.assert_array_equal(_upd(evs[t])[0], touched)
    assert evs[1].updated_count() == 0             # not in var_list: left alone
    assert len(evs[1].pending_grads) == 1
    opt.apply_gradients([evs[1]])                  # its formed slice: marked from sl.rows
    touched = np.unique(ids[:, 1])
    assert evs[1].updated_count() == touched.size
    np.testing.assert_array_equal(_upd(evs[1])[0], touched)
    dr.status_check()


# -- 6 -------------------------------------------------------------------------
def test_adagrad_by_row_equals_by_key():
    import deeprec_amd as dr
    batches = _batches(12)
    res = {}
    for by_row in (False, True):
        evs = _tables(dr, "rowmark_ada_%d" % by_row)
        for ev in evs:
            ev.track_updates(by_row=by_row)
        opt = dr.AdagradOptimizer(0.05)
        for s, batch in enumerate(batches):
            _step(dr, evs, opt, batch, s + 1)
        slots = [ev.slot("Adagrad", 0.1) for ev in evs]
        res[by_row] = ([_snap(ev) for ev in evs + slots], [_upd(ev) for ev in evs + slots],
                       [ev.updated_count() for ev in evs])
    for x, y in zip(res[False][0] + res[False][1], res[True][0] + res[True][1]):
        _same(x, y)
    assert res[False][2] == res[True][2]
    assert res[True][2] == [_touched(batches, f).size for f in range(2)]
    dr.status_check()


# -- 7 -------------------------------------------------------------------------
def test_mixed_group_by_row_and_by_key():
    import deeprec_amd as dr
    T = 2
    (ids, g), = _onehot_batches(14, T, steps=1)
    evs = [_table(dr, "rowmark_mix_%d" % t, BASE, 60 + t) for t in range(T)]
    evs[0].track_updates(by_row=True)
    evs[1].track_updates()
    assert evs[0].tracking_by_row() and not evs[1].tracking_by_row()
    opt = dr.GradientDescentOptimizer(0.05)
    pend = _onehot_step(dr, evs, ids, g, opt, evs)
    assert len({id(p._pending) for p in pend}) == 1
    assert not pend[0]._pending.applied            # the by-key member formed the gradient
    assert all(not ev.pending_grads for ev in evs)
    for t in range(T):
        touched = np.unique(ids[:, t])
        assert evs[t].updated_count() == touched.size
        np.testing.assert_array_equal(_upd(evs[t])[0], touched)
    dr.status_check()


# -- 8 -------------------------------------------------------------------------
def test_delta_of_a_by_row_trainer_brings_a_replica_up_to_date(tmp_path):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    a = _tables(dr, "rowmark_e2e_a", steps_to_live=1000)
    b = [dr.EmbeddingVariable("rowmark_e2e_b_%d" % f, D, 0.05, device=DEV, capacity=1024,
                              steps_to_live=1000) for f in range(2)]
    va = {"emb%d" % f: ev for f, ev in enumerate(a)}
    vb = {"emb%d" % f: ev for f, ev in enumerate(b)}
    full = ck.save(str(tmp_path / "full"), va)
    ck.restore(full, vb)
    for ev in a:
        ev.track_updates(by_row=True)
    opt = dr.GradientDescentOptimizer(0.05)
    batches = _batches(15)
    for s, batch in enumerate(batches):
        pend = _step(dr, a, opt, batch, s + 1)
        assert all(p._pending.applied for p in pend)
    for f in range(2):
        assert a[f].updated_count() == _touched(batches, f).size
    delta = ck.save_incremental(str(tmp_path / "delta"), va, global_step=3)
    r = ck.BundleReader(delta)
    for f in range(2):
        np.testing.assert_array_equal(np.sort(r.lookup("emb%d-sparse_incr_keys" % f)),
                                      _touched(batches, f))
    ck.restore_incremental(delta, vb)
    for n in va:
        sa, sb = _snap(va[n]), _snap(vb[n])
        assert sa[2].size == sa[0].size and sa[2].max() == 3      # versions are kept and stamped
        _same(sb, sa)
    again = ck.save_incremental(str(tmp_path / "delta2"), va)
    r2 = ck.BundleReader(again)
    for n in va:
        assert va[n].updated_count() == 0
        assert r2.dtype_and_shape(n + "-sparse_incr_keys")[1] == (0,)
    dr.status_check()


# -- 9 -------------------------------------------------------------------------
def test_rows_after_a_compaction():
    import deeprec_amd as dr
    batches = _batches(16, steps=2)
    res = {}
    for by_row in (False, True):
        evs = _tables(dr, "rowmark_cmp_%d" % by_row, steps_to_live=5)
        for ev in evs:
            ev.track_updates(by_row=by_row)
        opt = dr.GradientDescentOptimizer(0.05)
        _step(dr, evs, opt, batches[0], 4)
        for ev in evs:
            before = ev.total_count()[0].item()
            assert 0 < ev.shrink(7) < before       # the untouched base keys (version 0) go
            assert ev.compact() > 0                # ... and the kept keys change rows
        pend = _step(dr, evs, opt, batches[1], 8)
        assert all(p._pending.applied for p in pend) == by_row
        res[by_row] = ([_upd(ev) for ev in evs], [_snap(ev) for ev in evs],
                       [ev.updated_count() for ev in evs])
    for x, y in zip(res[False][0] + res[False][1], res[True][0] + res[True][1]):
        _same(x, y)
    assert res[False][2] == res[True][2]
    assert all(u[0].size > 0 for u in res[True][0])
    dr.status_check()
