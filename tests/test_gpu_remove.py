"""Keyed removal from an EmbeddingVariable's key space (dr_ev_remove) on the GPU.

The reference is the EV's own export() before the call, minus the removed
keys.  After every remove: export() of every column (keys, values bitwise,
versions, freqs), total_count(), and find() on all original keys -- a removed
key gives a negative result, a survivor the row it had before.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _bits(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy()
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _snap(ev):
    k, v, ve, fr = ev.export()
    return k.cpu().numpy(), _bits(v), ve.cpu().numpy(), fr.cpu().numpy()


def _same(got, ref):
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (g.dtype, g.shape, r.dtype, r.shape)
        np.testing.assert_array_equal(g, r)


def _minus(snap, gone):
    """The reference: a snapshot without the keys in `gone`."""
    keep = ~np.isin(snap[0], gone)
    return tuple(a[keep] if a.shape[0] == keep.size else a for a in snap)


def _state(cols, keys):
    return {"export": [_snap(c) for c in cols],
            "rows": [c.find(_t(keys)).cpu().numpy() for c in cols],
            "count": int(cols[0].total_count()[0])}


def _remove_and_check(cols, keys, gone, listed=None):
    """remove(listed or gone) on cols[0]'s key space; `gone` = the distinct
    keys of the list that are in the map.  Returns the state afterwards."""
    before = _state(cols, keys)
    present = np.isin(keys, gone)
    got = cols[0].remove(_t(gone if listed is None else listed))
    assert got == np.unique(gone).size
    after = _state(cols, keys)
    assert after["count"] == before["count"] - got
    for c in range(len(cols)):
        _same(after["export"][c], _minus(before["export"][c], gone))
        assert (after["rows"][c][present] < 0).all()
        np.testing.assert_array_equal(after["rows"][c][~present], before["rows"][c][~present])
    return after


def _mix64(k):
    """The table's hash (dr_common.h mix64), restated."""
    k = np.asarray(k).astype(np.uint64)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    return k ^ (k >> np.uint64(33))


def _random_keys(rng, n):
    k = np.unique(rng.integers(-2**62, 2**62, 2 * n + 16).astype(np.int64))
    k = k[(k != -1) & (k != 0)]
    rng.shuffle(k)
    assert k.size >= n and (k[:n] < 0).any()
    return k[:n]


SLOTS = 1024     # capacity 512 -> next_pow2(max(1024, 2 * 512)) slots, the minimum (dr_ev_create)


def _clustered_keys(rng, n, crowd):
    """n distinct keys of which `crowd` have their home slot in 8 chosen
    128-B lines (64 slots): they chain far past their home lines."""
    lines = rng.choice(SLOTS // 8, 8, replace=False)
    cand = _random_keys(rng, 40 * crowd)
    home_line = (_mix64(cand) & np.uint64(SLOTS - 1)) >> np.uint64(3)
    inside = np.isin(home_line, lines.astype(np.uint64))
    assert inside.sum() >= crowd
    crowded = cand[inside][:crowd]
    rest = cand[~inside][:n - crowd]
    keys = np.concatenate([crowded, rest])
    rng.shuffle(keys)
    hl = (_mix64(keys) & np.uint64(SLOTS - 1)) >> np.uint64(3)
    assert np.isin(hl, lines.astype(np.uint64)).sum() >= 200 and np.unique(keys).size == n
    return keys


@pytest.mark.parametrize("clustered", [False, True])
def test_probe_chains_survive(clustered):
    """Linear probing's deletion hazard: a survivor behind a removed key of
    its chain must still be found (load 700 / 1024, below the 3/4 growth)."""
    import deeprec_amd as dr
    rng = np.random.default_rng(31 + clustered)
    keys = _clustered_keys(rng, 700, 220) if clustered else _random_keys(rng, 700)
    ev = dr.EmbeddingVariable("rm_chain_%d" % clustered, 4, 0.5, capacity=512, device=DEV)
    assert dr._lib.lib().dr_ev_row_capacity(ev.handle) == 1024
    ev.insert(_t(keys), _t(rng.standard_normal((700, 4)).astype(np.float32)))
    assert dr._lib.lib().dr_ev_row_capacity(ev.handle) == 1024      # no growth: still 1024 slots
    after = _remove_and_check([ev], keys, keys[::3])
    assert after["count"] == 700 - keys[::3].size
    # and once more on the rehashed table
    rest = keys[np.arange(700) % 3 != 0]
    _remove_and_check([ev], keys, rest[::2])
    dr.status_check()


@pytest.mark.parametrize("victim", [-1, 0])
def test_special_keys(victim):
    """Key -1 lives in the special slot at index cap, key 0 is an ordinary
    key: each goes without the other."""
    import deeprec_amd as dr
    keys = np.array([5, -1, 17, 0, -9], np.int64)
    ev = dr.EmbeddingVariable("rm_special_%d" % (victim + 1), 4, 0.5, steps_to_live=4,
                              capacity=512, device=DEV)
    ev.insert(_t(keys), _t(np.arange(20, dtype=np.float32).reshape(5, 4)),
              _t(np.arange(5, dtype=np.int64)))
    after = _remove_and_check([ev], keys, np.array([victim], np.int64))
    other = -1 - victim
    assert other in after["export"][0][0].tolist() and victim not in after["export"][0][0].tolist()
    _remove_and_check([ev], keys, np.array([other], np.int64))
    dr.status_check()


def test_remove_list_shapes():
    import deeprec_amd as dr
    rng = np.random.default_rng(3)
    keys = np.concatenate([_random_keys(rng, 298), np.array([-1, 0], np.int64)])
    ev = dr.EmbeddingVariable("rm_shapes", 4, 0.5, capacity=512, device=DEV)
    ev.insert(_t(keys), _t(rng.standard_normal((300, 4)).astype(np.float32)))
    # duplicates: `removed` counts distinct keys (the same key within a wave and across blocks)
    gone = keys[:40]
    listed = np.concatenate([gone, gone[:7], np.repeat(gone[3], 600), gone[::-1]])
    _remove_and_check([ev], keys, gone, listed)
    # absent keys (never inserted, and the ones just removed) are ignored
    absent = np.arange(10**12, 10**12 + 50, dtype=np.int64)
    gone2 = keys[40:60]
    _remove_and_check([ev], keys, gone2, np.concatenate([absent, gone2, gone]))
    before = _state([ev], keys)
    assert ev.remove(_t(absent)) == 0
    _same(_snap(ev), before["export"][0])
    # n = 0
    assert ev.remove(_t(np.zeros(0, np.int64))) == 0
    _same(_snap(ev), before["export"][0])
    # everything
    after = _remove_and_check([ev], keys, keys[60:], keys)
    assert after["export"][0][0].size == 0 and after["count"] == 0
    assert ev.rows_allocated() == 300
    dr.status_check()


@pytest.mark.parametrize("dim,vdt", [(4, torch.float32), (128, torch.float32),
                                     (128, torch.bfloat16), (8, torch.float64)])
def test_widths_and_columns(dim, vdt):
    """Every value width, with an Adagrad slot column on every second key:
    the key goes from both columns."""
    import deeprec_amd as dr
    rng = np.random.default_rng(dim)
    n = 600
    keys = _random_keys(rng, n)
    ev = dr.EmbeddingVariable("rm_width_%d_%s" % (dim, vdt), dim, 0.5, steps_to_live=3,
                              capacity=512, device=DEV, value_dtype=vdt)
    acc = ev.slot("Adagrad", 0.1)
    np_dt = np.float64 if vdt == torch.float64 else np.float32
    ev.insert(_t(keys), _t(rng.standard_normal((n, dim)).astype(np_dt)),
              _t(rng.integers(0, 50, n).astype(np.int64)))
    acc.insert(_t(keys[::2]), _t(rng.standard_normal((keys[::2].size, dim)).astype(np_dt)))
    before = _state([ev, acc], keys)
    assert before["export"][0][0].size == n and before["export"][1][0].size == keys[::2].size
    after = _remove_and_check([ev, acc], keys, keys[::3])
    gone_acc = np.intersect1d(keys[::3], keys[::2]).size
    assert gone_acc > 50 and after["export"][1][0].size == keys[::2].size - gone_acc
    dr.status_check()


def test_counter_filter_key_below_the_threshold():
    """Neither the first-touch bits nor the Counter rule is consulted."""
    import deeprec_amd as dr
    opt = dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(filter_freq=3))
    ev = dr.EmbeddingVariable("rm_counter", 4, 0.5, capacity=512, device=DEV, ev_option=opt)
    seen3, seen1 = np.arange(10, 20, dtype=np.int64), np.arange(100, 105, dtype=np.int64)
    for _ in range(4):
        ev.sparse_read(_t(seen3))
    ev.sparse_read(_t(seen1))
    assert ev.key_meta(seen1)[0].tolist() == [1] * 5        # in the map (counted), not admitted
    assert (ev.find(_t(seen1)) < 0).all() and int(ev.total_count()[0]) == 15
    keys = np.concatenate([seen3, seen1])
    before = _state([ev], keys)
    assert ev.remove(_t(seen1[:2])) == 2
    assert int(ev.total_count()[0]) == 13
    assert ev.key_meta(seen1)[0].tolist() == [0, 0, 1, 1, 1]    # gone from the map
    after = _state([ev], keys)
    _same(after["export"][0], _minus(before["export"][0], seen1[:2]))
    np.testing.assert_array_equal(after["rows"][0], before["rows"][0])
    assert (after["rows"][0][:10] >= 0).all()
    # the removed key counts from zero again
    ev.sparse_read(_t(seen1[:1]))
    assert ev.key_meta(seen1[:1])[0].tolist() == [1]
    dr.status_check()


def test_reinsert_gets_a_fresh_row():
    import deeprec_amd as dr
    rng = np.random.default_rng(12)
    keys = _random_keys(rng, 100)
    ev = dr.EmbeddingVariable("rm_reinsert", 4, 0.25, steps_to_live=5, capacity=512, device=DEV)
    ev.insert(_t(keys), _t(rng.standard_normal((100, 4)).astype(np.float32)),
              _t(np.full(100, 7, np.int64)), _t(np.full(100, 9, np.int64)))
    rows = ev.find(_t(keys)).cpu().numpy()
    _remove_and_check([ev], keys, keys[:1])
    assert ev.rows_allocated() == 100
    fresh = np.array([10**15], np.int64)                    # never seen: what "fresh" means
    out = ev.sparse_read(_t(np.concatenate([keys[:1], fresh])))
    np.testing.assert_array_equal(out.cpu().numpy(), np.full((2, 4), 0.25, np.float32))
    assert ev.rows_allocated() == 102                       # one new row each
    fr, ve, has = ev.key_meta(np.concatenate([keys[:1], fresh]))
    assert has.all() and fr[0] == fr[1] and ve[0] == ve[1] and fr[0] != 9 and ve[0] != 7
    r = ev.find(_t(keys[:1])).item()
    assert r >= 100 and r != rows[0]
    dr.status_check()


def test_remove_then_compact():
    import deeprec_amd as dr
    rng = np.random.default_rng(13)
    n = 900
    keys = _random_keys(rng, n)
    ev = dr.EmbeddingVariable("rm_compact", 8, 0.5, steps_to_live=3, capacity=1024, device=DEV)
    acc = ev.slot("Adagrad", 0.1)
    ev.insert(_t(keys), _t(rng.standard_normal((n, 8)).astype(np.float32)),
              _t(rng.integers(0, 50, n).astype(np.int64)))
    acc.insert(_t(keys[::2]), _t(rng.standard_normal((keys[::2].size, 8)).astype(np.float32)))
    ev.track_updates()
    ev.mark_updated(_t(keys[::4]))
    gone = keys[rng.random(n) < 0.4]
    mid = _remove_and_check([ev, acc], keys, gone)
    upd = (_snap_updated(ev), _snap_updated(acc))
    assert ev.rows_allocated() == n
    assert ev.compact() == gone.size
    assert ev.rows_allocated() == int(ev.total_count()[0]) == n - gone.size
    after = _state([ev, acc], keys)
    for c in range(2):
        _same(after["export"][c], mid["export"][c])
        assert ((after["rows"][c] < 0) == (mid["rows"][c] < 0)).all()
    _same(_snap_updated(ev), upd[0])
    _same(_snap_updated(acc), upd[1])
    dr.status_check()


def _snap_updated(ev):
    k, v, ve, fr = ev.export_updated()
    return k.cpu().numpy(), _bits(v), ve.cpu().numpy(), fr.cpu().numpy()


def test_growth_afterwards():
    import deeprec_amd as dr
    rng = np.random.default_rng(14)
    allk = _random_keys(rng, 3700)
    keys, more = allk[:700], allk[700:]
    ev = dr.EmbeddingVariable("rm_grow", 4, 0.5, capacity=512, device=DEV)
    vals = rng.standard_normal((3700, 4)).astype(np.float32)
    ev.insert(_t(keys), _t(vals[:700]))
    cap0 = dr._lib.lib().dr_ev_row_capacity(ev.handle)
    gone = keys[::3]
    mid = _remove_and_check([ev], keys, gone)
    ev.insert(_t(more), _t(vals[700:]))                     # slot table and row pool both grow
    assert dr._lib.lib().dr_ev_row_capacity(ev.handle) > cap0
    rows = ev.find(_t(allk)).cpu().numpy()
    present = ~np.isin(allk, gone)
    assert (rows[present] >= 0).all() and (rows[~present] < 0).all()
    np.testing.assert_array_equal(rows[:700][present[:700]], mid["rows"][0][present[:700]])
    assert np.unique(rows[present]).size == present.sum()
    k, v, _, _ = _snap(ev)
    o = np.argsort(allk[present])
    np.testing.assert_array_equal(k, allk[present][o])
    np.testing.assert_array_equal(v, vals[present][o].view(np.uint32))
    assert int(ev.total_count()[0]) == present.sum()
    dr.status_check()


def test_refusals():
    import deeprec_amd as dr
    from deeprec_amd._lib import INVALID_ARGUMENT, lib, stream_handle
    ev = dr.EmbeddingVariable("rm_refuse", 4, 0.5, capacity=512, device=DEV)
    acc = ev.slot("Adagrad", 0.1)
    keys = np.arange(10, dtype=np.int64)
    ev.sparse_read(_t(keys))
    dk = _t(keys[:3])
    n = C.c_int64(-5)
    # a slot EV handle
    assert lib().dr_ev_remove(acc.handle, dk.data_ptr(), 3, C.byref(n),
                              stream_handle(ev.device)) == INVALID_ARGUMENT
    assert lib().dr_last_error() and n.value == -5
    # inside stream capture: refused before anything is touched
    x = torch.zeros(8, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x += 1
        rc = lib().dr_ev_remove(ev.handle, dk.data_ptr(), 3, C.byref(n), stream_handle(ev.device))
    assert rc == INVALID_ARGUMENT and lib().dr_last_error()
    assert n.value == 0 and int(ev.total_count()[0]) == 10
    g.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 8
    # a queued gradient of the primary or of a slot
    sl = dr.IndexedSlices(_t(np.ones((10, 4), np.float32)), _t(keys))
    ev.pending_grads.append(sl)
    with pytest.raises(dr.InvalidArgumentError):
        ev.remove(dk)
    with pytest.raises(dr.InvalidArgumentError):
        acc.remove(dk)
    ev.pending_grads.clear()
    acc.pending_grads.append(sl)
    with pytest.raises(dr.InvalidArgumentError):
        ev.remove(dk)
    acc.pending_grads.clear()
    assert int(ev.total_count()[0]) == 10
    assert acc.remove(dk) == 3                               # through the primary
    assert ev.export()[0].tolist() == list(range(3, 10))
    dr.status_check()
