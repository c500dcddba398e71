"""Update tracking, delta export and upsert of an EmbeddingVariable on the GPU.

The reference everywhere is the engine's own full export(): export_updated()
must equal export() filtered on the host to the marked keys that are present
-- keys, values bit for bit, versions, freqs and order -- and none of the new
calls may change what export() returns.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SPECIAL = np.array([-1, 0, -2, 2**63 - 1, -2**63, -7, -1000, -123456789], np.int64)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _bits(t):
    """Values as integers of their own width: the comparison is bitwise."""
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy()
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _snap(four):
    k, v, ve, fr = four
    return k.cpu().numpy(), _bits(v), ve.cpu().numpy(), fr.cpu().numpy()


def _filtered(full, marked):
    k, v, ve, fr = full
    sel = np.isin(k, np.asarray(marked, np.int64))
    return k[sel], v[sel], ve[sel] if ve.size else ve, fr[sel] if fr.size else fr


def _same(got, ref):
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (g.dtype, g.shape, r.dtype, r.shape)
        np.testing.assert_array_equal(g, r)


def _keys(rng, n):
    body = np.unique(rng.integers(1, 1 << 40, 2 * n).astype(np.int64))
    body = body[~np.isin(body, SPECIAL)]
    rng.shuffle(body)
    keys = np.concatenate([SPECIAL, body[:n - SPECIAL.size]])
    assert np.unique(keys).size == n
    return keys


def _fill(ev, rng, keys, chunks=1, dtype=np.float32, **kw):
    vals = rng.standard_normal((keys.size, ev.dim)).astype(dtype)
    for part in np.array_split(np.arange(keys.size), chunks):
        extra = {k: _t(v[part]) for k, v in kw.items()}
        ev.insert(_t(keys[part]), _t(vals[part]), **extra)
    return vals


@pytest.mark.parametrize("dim,short", [(1, False), (6, False), (6, True), (16, False),
                                       (128, False)])
def test_export_updated_is_the_filtered_full_export(dim, short):
    import deeprec_amd as dr
    rng = np.random.default_rng(100 + dim)
    ev = dr.EmbeddingVariable("incr_exp_%d_%d" % (dim, short), dim, 0.5, device=DEV, capacity=64)
    keys = _keys(rng, 3000)
    cap0 = dr._lib.lib().dr_ev_row_capacity(ev.handle)
    _fill(ev, rng, keys, chunks=5)
    assert dr._lib.lib().dr_ev_row_capacity(ev.handle) > cap0      # it grew on the way
    before = _snap(ev.export())
    count = ev.total_count().tolist()
    assert count[0] == 3000
    ev.track_updates()
    assert ev.tracking_updates()
    marked = np.concatenate([SPECIAL, rng.permutation(keys[SPECIAL.size:])[:1100 - SPECIAL.size]])
    absent = -(np.arange(150, dtype=np.int64) + 5) * 1000003      # none of them is a key
    assert not np.isin(absent, keys).any()
    lst = np.concatenate([marked, marked[rng.integers(0, marked.size, 200)], absent])
    rng.shuffle(lst)
    n_dev = None
    if short:
        n_dev = torch.tensor([1000], dtype=torch.int64, device=DEV)
        lst_eff = lst[:1000]
    else:
        lst_eff = lst
    ev.mark_updated(_t(lst), n_dev)
    got = _snap(ev.export_updated())
    ref = _filtered(before, lst_eff)
    m = ref[0].size
    assert m == np.unique(lst_eff[np.isin(lst_eff, keys)]).size and m > 0
    if not short:
        assert m == 1100
    _same(got, ref)
    assert ev.total_count().tolist() == count                      # absent keys were not created
    assert ev.updated_count() == m
    ev.clear_updated()
    ev.track_updates(False)
    _same(_snap(ev.export()), before)                              # nothing changed the table


def _edge_ev(name):
    import deeprec_amd as dr
    ev = dr.EmbeddingVariable(name, 4, 0.25, device=DEV, capacity=1024)
    keys = np.arange(200, dtype=np.int64)
    rng = np.random.default_rng(7)
    _fill(ev, rng, keys)
    rows = ev.find(_t(keys)).cpu().numpy()
    assert sorted(rows.tolist()) == list(range(200))               # rows 0..199, one per key
    return ev, keys, rows


def test_bit_and_word_edges():
    ev, keys, rows = _edge_ev("incr_edges")
    full = _snap(ev.export())
    ev.track_updates()
    want_rows = np.array([0, 31, 32, 63, 64, 65, 127, 128])
    marked = keys[np.isin(rows, want_rows)]
    assert marked.size == want_rows.size
    ev.mark_updated(_t(marked))
    _same(_snap(ev.export_updated()), _filtered(full, marked))
    assert ev.updated_count() == want_rows.size
    _same(_snap(ev.export()), full)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_mark_counts_around_a_wave(n):
    ev, keys, _ = _edge_ev("incr_wave_%d" % n)
    full = _snap(ev.export())
    ev.track_updates()
    marked = np.random.default_rng(n).permutation(keys)[:n]
    ev.mark_updated(_t(marked))
    got = _snap(ev.export_updated())
    assert got[0].size == n and got[1].shape == (n, 4)
    _same(got, _filtered(full, marked))
    assert ev.updated_count() == n


def test_growth_while_tracking_keeps_the_marks():
    import deeprec_amd as dr
    rng = np.random.default_rng(21)
    ev = dr.EmbeddingVariable("incr_grow", 6, 0.5, device=DEV, capacity=1024)
    keys = _keys(rng, 5000)
    old, new = keys[:1000], keys[1000:]
    _fill(ev, rng, old)
    ev.track_updates()
    m1 = rng.permutation(old)[:500]
    ev.mark_updated(_t(m1))
    cap0 = dr._lib.lib().dr_ev_row_capacity(ev.handle)
    _fill(ev, rng, new, chunks=2)
    assert dr._lib.lib().dr_ev_row_capacity(ev.handle) > cap0
    m2 = rng.permutation(new)[:300]
    ev.mark_updated(_t(m2))
    full = _snap(ev.export())
    assert full[0].size == 5000
    got = _snap(ev.export_updated())
    assert got[0].size == 800
    _same(got, _filtered(full, np.concatenate([m1, m2])))
    assert ev.updated_count() == 800


def test_grouped_mark_over_several_tables():
    """One launch over three tables of different dims: a device count on the
    first, the second not tracking (skipped), the third empty-handed."""
    import deeprec_amd as dr
    from deeprec_amd.kv_variable_ops import mark_updated_grouped
    rng = np.random.default_rng(41)
    evs, keys, fulls = [], [], []
    for t, dim in enumerate((4, 6, 16)):
        ev = dr.EmbeddingVariable("incr_grp_%d" % t, dim, 0.5, device=DEV, capacity=1024)
        k = _keys(rng, 700 + 100 * t)
        _fill(ev, rng, k)
        evs.append(ev)
        keys.append(k)
        fulls.append(_snap(ev.export()))
    evs[0].track_updates()
    evs[2].track_updates()
    lists = [rng.permutation(keys[0])[:300], rng.permutation(keys[1])[:200],
             rng.permutation(keys[2])[:257]]
    nd = [torch.tensor([129], dtype=torch.int64, device=DEV), None, None]
    # the C entry itself over all three (the second table's key space is not tracking) ...
    from deeprec_amd._lib import lib, stream_handle
    flat = _t(np.concatenate([x[:100] for x in lists]))
    handles = (C.c_void_p * 3)(*[ev.handle.value for ev in evs])
    koff = (C.c_int64 * 4)(0, 100, 200, 300)
    assert lib().dr_ev_mark_updated(handles, 3, flat.data_ptr(), koff, None,
                                    stream_handle(evs[0].device)) == 0
    assert evs[0].updated_count() == 100 and evs[2].updated_count() == 100
    # ... and the Python grouping, which leaves that table out
    mark_updated_grouped(evs, [_t(x) for x in lists], nd)
    _same(_snap(evs[0].export_updated()), _filtered(fulls[0], lists[0][:129]))
    _same(_snap(evs[2].export_updated()), _filtered(fulls[2], lists[2]))
    assert evs[0].updated_count() == 129 and evs[2].updated_count() == 257
    assert not evs[1].tracking_updates()
    for ev, full in zip(evs, fulls):
        _same(_snap(ev.export()), full)


@pytest.mark.parametrize("vdt,dim", [(torch.float32, 8), (torch.bfloat16, 16), (torch.float64, 4)])
def test_slots_and_value_types(vdt, dim):
    import deeprec_amd as dr
    rng = np.random.default_rng(dim)
    ev = dr.EmbeddingVariable("incr_slot_%d" % dim, dim, 0.5, device=DEV, capacity=1024,
                              value_dtype=vdt)
    acc = ev.slot("Adagrad", 0.1)
    keys = _keys(rng, 1500)
    np_dt = np.float64 if vdt == torch.float64 else np.float32
    _fill(ev, rng, keys, dtype=np_dt)
    touched = keys[:700]                       # the accumulator column of these keys only
    _fill(acc, rng, touched, dtype=np_dt)
    full_p, full_a = _snap(ev.export()), _snap(acc.export())
    assert full_p[0].size == 1500 and full_a[0].size == 700
    acc.track_updates()                        # on a slot: the shared key space
    assert ev.tracking_updates()
    marked = np.concatenate([keys[400:1000], SPECIAL])
    ev.mark_updated(_t(marked))
    got_p, got_a = _snap(ev.export_updated()), _snap(acc.export_updated())
    _same(got_p, _filtered(full_p, marked))
    _same(got_a, _filtered(full_a, marked))
    # a column not yet touched for a key drops the key from that column only
    assert got_p[0].size == np.unique(marked).size
    assert got_a[0].size == np.isin(np.unique(marked), touched).sum() < got_p[0].size
    assert ev.updated_count() == got_p[0].size
    _same(_snap(ev.export()), full_p)
    _same(_snap(acc.export()), full_a)


def test_versions_are_exported():
    import deeprec_amd as dr
    rng = np.random.default_rng(31)
    ev = dr.EmbeddingVariable("incr_ver", 6, 0.5, device=DEV, capacity=1024, steps_to_live=5)
    keys = _keys(rng, 1200)
    _fill(ev, rng, keys, versions=rng.integers(0, 100, keys.size).astype(np.int64))
    full = _snap(ev.export())
    assert full[2].size == 1200 and np.unique(full[2]).size > 10
    ev.track_updates()
    marked = rng.permutation(keys)[:400]
    ev.mark_updated(_t(marked))
    got = _snap(ev.export_updated())
    assert got[2].size == 400
    _same(got, _filtered(full, marked))


def test_counter_filter_keeps_unadmitted_keys_out():
    import deeprec_amd as dr
    rng = np.random.default_rng(32)
    opt = dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(filter_freq=3))
    ev = dr.EmbeddingVariable("incr_cnt", 6, 0.5, device=DEV, capacity=1024, ev_option=opt)
    keys = _keys(rng, 1000)
    _fill(ev, rng, keys, freqs=rng.integers(0, 9, keys.size).astype(np.int64))   # admitted
    seen_once = np.arange(1, 201, dtype=np.int64) * -1000003                      # freq 1 < 3
    assert not np.isin(seen_once, keys).any()
    ev.sparse_read(_t(seen_once))
    full = _snap(ev.export())
    assert full[0].size == 1000 and full[3].size == 1000
    ev.track_updates()
    marked = np.concatenate([rng.permutation(keys)[:300], seen_once])
    ev.mark_updated(_t(marked))
    got = _snap(ev.export_updated())
    assert got[0].size == 300 and not np.isin(got[0], seen_once).any()
    _same(got, _filtered(full, marked))
    _same(_snap(ev.export()), full)


def test_shrink_between_mark_and_export():
    import deeprec_amd as dr
    rng = np.random.default_rng(33)
    ev = dr.EmbeddingVariable("incr_shrink", 6, 0.5, device=DEV, capacity=1024, steps_to_live=5)
    keys = _keys(rng, 1500)
    _fill(ev, rng, keys, versions=rng.integers(0, 21, keys.size).astype(np.int64))
    ev.track_updates()
    marked = rng.permutation(keys)[:500]
    ev.mark_updated(_t(marked))
    removed = ev.shrink(global_step=20)                  # drops versions < 15
    assert 0 < removed < 1500
    full = _snap(ev.export())
    assert full[0].size == 1500 - removed
    got = _snap(ev.export_updated())
    _same(got, _filtered(full, marked))
    m = got[0].size
    assert 0 < m < 500                                   # some marked keys were evicted
    assert ev.updated_count() == 500 >= m                # an upper bound: their bits stay


def test_clear_stop_and_bloom():
    import deeprec_amd as dr
    rng = np.random.default_rng(34)
    ev = dr.EmbeddingVariable("incr_clear", 6, 0.5, device=DEV, capacity=1024)
    keys = _keys(rng, 600)
    _fill(ev, rng, keys)
    full = _snap(ev.export())
    ev.track_updates()
    ev.track_updates()                                   # idempotent
    ev.mark_updated(_t(keys[:100]))
    assert ev.updated_count() == 100
    ev.clear_updated()
    k, v, ve, fr = ev.export_updated()
    assert k.shape == (0,) and v.shape == (0, 6) and ve.shape == (0,) and fr.shape == (0,)
    assert k.dtype == torch.int64 and v.dtype == torch.float32
    assert ev.updated_count() == 0
    ev.mark_updated(_t(keys[50:250]))                    # marking again works
    _same(_snap(ev.export_updated()), _filtered(full, keys[50:250]))
    ev.track_updates(False)
    ev.track_updates(False)
    assert not ev.tracking_updates()
    with pytest.raises(dr.InvalidArgumentError):
        ev.export_updated()
    with pytest.raises(dr.InvalidArgumentError):
        ev.updated_count()
    ev.mark_updated(_t(keys[:10]))                       # a no-op
    ev.track_updates()
    assert ev.updated_count() == 0                       # a fresh bitmap
    _same(_snap(ev.export()), full)
    bloom = dr.EmbeddingVariable(
        "incr_bloom", 6, 0.5, device=DEV, capacity=1024,
        ev_option=dr.EmbeddingVariableOption(filter_option=dr.CBFFilter(
            filter_freq=3, max_element_size=1000, false_positive_probability=0.01)))
    with pytest.raises(dr.InvalidArgumentError):
        bloom.track_updates()
    assert not bloom.tracking_updates()
    i32 = dr.EmbeddingVariable("incr_i32", 6, 0.5, device=DEV, capacity=1024,
                               key_dtype=torch.int32)
    with pytest.raises(dr.InvalidArgumentError):
        i32.track_updates()


def test_export_capacity_is_checked():
    import deeprec_amd as dr
    from deeprec_amd._lib import INVALID_ARGUMENT, lib, ptr, stream_handle
    rng = np.random.default_rng(35)
    ev = dr.EmbeddingVariable("incr_capacity", 6, 0.5, device=DEV, capacity=1024)
    keys = _keys(rng, 300)
    _fill(ev, rng, keys)
    ev.track_updates()
    ev.mark_updated(_t(keys[:40]))
    m = C.c_int64(0)
    st = stream_handle(ev.device)
    assert lib().dr_ev_export_updated(ev.handle, None, None, None, None, 0, C.byref(m), st) == 0
    assert m.value == 40
    k = torch.empty(40, dtype=torch.int64, device=DEV)
    v = torch.empty((40, 6), dtype=torch.float32, device=DEV)
    assert lib().dr_ev_export_updated(ev.handle, ptr(k), ptr(v), None, None, 39, C.byref(m),
                                      st) == INVALID_ARGUMENT
    assert lib().dr_last_error()
    assert lib().dr_ev_export_updated(ev.handle, ptr(k), ptr(v), None, None, 40, C.byref(m),
                                      st) == 0
    full = _snap(ev.export())
    ref = _filtered(full, keys[:40])
    np.testing.assert_array_equal(k.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(_bits(v), ref[1])


def _filter_ev(dr, name):
    opt = dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(filter_freq=3))
    return dr.EmbeddingVariable(name, 6, 0.5, device=DEV, capacity=1024, steps_to_live=5,
                                ev_option=opt)


def test_upsert_overwrites_where_insert_keeps():
    import deeprec_amd as dr
    rng = np.random.default_rng(36)
    keys = _keys(rng, 2000)
    have, new = keys[:1000], keys[1000:1500]
    inp = np.concatenate([have[:500], new])
    rng.shuffle(inp)
    v0 = rng.standard_normal((have.size, 6)).astype(np.float32)
    v1 = rng.standard_normal((inp.size, 6)).astype(np.float32)
    ver0 = rng.integers(0, 50, have.size).astype(np.int64)
    ver1 = rng.integers(50, 99, inp.size).astype(np.int64)
    fr1 = rng.integers(0, 9, inp.size).astype(np.int64)
    a, b = _filter_ev(dr, "incr_up_a"), _filter_ev(dr, "incr_up_b")
    for ev in (a, b):
        ev.insert(_t(have), _t(v0), _t(ver0))
    a.upsert(_t(inp), _t(v1), _t(ver1), _t(fr1))
    b.insert(_t(inp), _t(v1), _t(ver1), _t(fr1))
    ka, va, vea, fra = _snap(a.export())
    kb, vb, veb, frb = _snap(b.export())
    want = np.sort(np.concatenate([have, new]))
    np.testing.assert_array_equal(ka, want)
    np.testing.assert_array_equal(kb, want)
    np.testing.assert_array_equal(vea, veb)          # versions and freqs: as insert stores them
    np.testing.assert_array_equal(fra, frb)
    old_rows = dict(zip(have.tolist(), v0.view(np.uint32)))
    new_rows = dict(zip(inp.tolist(), v1.view(np.uint32)))
    exp_a = np.stack([new_rows.get(k, old_rows.get(k)) for k in want.tolist()])
    exp_b = np.stack([old_rows[k] if k in old_rows else new_rows[k] for k in want.tolist()])
    np.testing.assert_array_equal(va, exp_a)         # upsert: the existing rows are overwritten
    np.testing.assert_array_equal(vb, exp_b)         # insert: they are kept
    assert (exp_a != exp_b).any()


@pytest.mark.parametrize("vdt,dim", [(torch.float32, 6), (torch.bfloat16, 16), (torch.float64, 4)])
def test_upsert_into_a_fresh_ev_is_insert(vdt, dim):
    """Partition filter, versions, freqs and new keys: on an empty EV upsert
    and the partitioned import are the same operation."""
    import deeprec_amd as dr
    rng = np.random.default_rng(37 + dim)
    keys = _keys(rng, 1200)
    vals = rng.standard_normal((keys.size, dim)).astype(
        np.float64 if vdt == torch.float64 else np.float32)
    vers = rng.integers(0, 50, keys.size).astype(np.int64)
    frqs = rng.integers(0, 9, keys.size).astype(np.int64)
    opt = dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(filter_freq=3))
    mk = lambda n: dr.EmbeddingVariable(n, dim, 0.5, device=DEV, capacity=64, steps_to_live=5,
                                        ev_option=opt, value_dtype=vdt)
    a, b = mk("incr_upf_a_%d" % dim), mk("incr_upf_b_%d" % dim)
    a._upsert(_t(keys), _t(vals), _t(vers), _t(frqs), 1, 3)
    b.import_partitioned(_t(keys), _t(vals), _t(vers), _t(frqs), 1, 3)
    sa, sb = _snap(a.export()), _snap(b.export())
    c_rem = lambda k: np.fmod(np.fmod(k, 1000), 3)           # C++ remainder: negatives match none
    assert sa[0].size == (c_rem(keys) == 1).sum() > 0
    assert (c_rem(sa[0]) == 1).all() and (sa[0] >= 0).all()
    _same(sa, sb)
