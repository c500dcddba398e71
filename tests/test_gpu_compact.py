"""Row compaction of an EmbeddingVariable's key space (dr_ev_compact) on the GPU.

The reference everywhere is the EV's own state before the call, or a twin EV
that is never compacted: compaction may change the row numbers that find()
returns -- to exactly the predicted ones: live rows below the live count L
stay, the k-th smallest live row >= L takes the k-th smallest hole below L --
and nothing else that can be observed.  Comparisons are bitwise.
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
    """Values as integers of their own width: the comparison is bitwise."""
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy()
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _snap(four):
    k, v, ve, fr = four
    return k.cpu().numpy(), _bits(v), ve.cpu().numpy(), fr.cpu().numpy()


def _same(got, ref):
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (g.dtype, g.shape, r.dtype, r.shape)
        np.testing.assert_array_equal(g, r)


def _keys(rng, n, lo=-2**62, hi=2**62):
    """n distinct random keys, negative ones included, none of them -1."""
    k = np.unique(rng.integers(lo, hi, 2 * n + 16).astype(np.int64))
    k = k[k != -1]
    rng.shuffle(k)
    assert k.size >= n and (k[:n] < 0).any()
    return k[:n]


def _predict(rows, top):
    """New rows of the live rows `rows` (one per kept key) of [0, top)."""
    live = np.zeros(top, bool)
    live[rows] = True
    L = rows.size
    assert live.sum() == L                          # a row belongs to one key
    holes = np.flatnonzero(~live[:L])
    movers = np.flatnonzero(live[L:]) + L
    assert holes.size == movers.size
    remap = np.arange(top)
    remap[movers] = holes
    return remap[rows], L, movers.size


def _state(ev, acc, keys):
    """Everything a compaction must leave as it was (and the rows)."""
    s = {"rows": ev.find(_t(keys)).cpu().numpy(),
         "export": _snap(ev.export()),
         "meta": ev.key_meta(keys),
         "ro": _bits(ev.sparse_read(_t(keys).to(ev.key_dtype), read_only=True)),
         "count": ev.total_count().tolist()}
    if acc is not None:
        s["export_acc"] = _snap(acc.export())
        s["ro_acc"] = _bits(acc.sparse_read(_t(keys).to(ev.key_dtype), read_only=True))
    if ev.tracking_updates():
        s["updated"] = _snap(ev.export_updated())
        if acc is not None:
            s["updated_acc"] = _snap(acc.export_updated())
    return s


def _same_state(a, b, rows=True):
    assert a.keys() == b.keys()
    for name in a:
        if name == "rows":
            if rows:
                np.testing.assert_array_equal(a[name], b[name])
        elif name in ("ro", "ro_acc"):
            np.testing.assert_array_equal(a[name], b[name])
        elif name == "count":
            assert a[name] == b[name]
        else:
            _same(a[name], b[name])


GS = 10          # the step of the shrink
EVICT, KEEP = 3, 9   # versions: GS - 3 > 2 goes, GS - 9 <= 2 stays (steps_to_live 2)


def _versions(n):
    v = np.full(n, KEEP, np.int64)
    v[::3] = EVICT
    return v


def test_layout_and_contents():
    import deeprec_amd as dr
    rng = np.random.default_rng(2024)
    keys = np.concatenate([_keys(rng, 5000), np.array([-1], np.int64)])   # -1 is kept (5000 % 3)
    n = keys.size
    ev = dr.EmbeddingVariable("cmp_layout", 4, 0.5, steps_to_live=2, capacity=8192, device=DEV)
    vals = rng.standard_normal((n, 4)).astype(np.float32)
    ev.insert(_t(keys), _t(vals))
    # the slot column of every second key, by an Adagrad apply at step GS ...
    opt = dr.AdagradOptimizer(0.1)
    acc = ev.slot("Adagrad", 0.1)
    ev.pending_grads.append(dr.IndexedSlices(
        _t(rng.standard_normal((keys[::2].size, 4)).astype(np.float32)), _t(keys[::2])))
    opt.apply_gradients([ev], global_step=GS)
    # ... which stamped their versions: the explicit ones decide the eviction
    vers = _versions(n)
    ev.insert(_t(keys), _t(vals), _t(vers))
    ev.track_updates()
    ev.mark_updated(_t(keys[::5]))
    kept = vers == KEEP
    before = _state(ev, acc, keys)
    assert before["export"][0].size == n and before["export_acc"][0].size == keys[::2].size
    assert (before["rows"] >= 0).all() and ev.rows_allocated() == n
    assert ev.updated_count() == keys[::5].size == before["updated"][0].size

    assert ev.shrink(GS) == (~kept).sum() == 1667
    mid = _state(ev, acc, keys)
    np.testing.assert_array_equal(mid["rows"][kept], before["rows"][kept])   # shrink keeps rows
    assert (mid["rows"][~kept] < 0).all()
    assert ev.rows_allocated() == n and mid["count"][0] == n - 1667
    assert ev.updated_count() == keys[::5].size > mid["updated"][0].size     # dead bits stay set
    cap = dr._lib.lib().dr_ev_row_capacity(ev.handle)
    pool, pool_acc = ev.pool(), acc.pool()

    assert ev.compact() == 1667
    want, L, moved = _predict(mid["rows"][kept], n)
    assert L == 3334 and L % 32 != 0 and moved > 100
    assert ev.rows_allocated() == int(ev.total_count()[0]) == L
    after = _state(ev, acc, keys)
    np.testing.assert_array_equal(after["rows"][kept], want)
    np.testing.assert_array_equal(after["rows"][~kept], mid["rows"][~kept])  # -(i + 1)
    _same_state(after, mid, rows=False)
    # evicted keys read the default, in both columns
    assert (after["ro"][~kept] == np.float32(0.5).view(np.uint32)).all()
    assert (after["ro_acc"][~kept] == np.float32(0.1).view(np.uint32)).all()
    assert not after["meta"][2][~kept].any() and after["meta"][2][kept].all()
    # a bit moved with its key and the evicted keys' bits are gone
    assert ev.updated_count() == (kept[::5]).sum() == after["updated"][0].size
    # nothing was reallocated
    assert dr._lib.lib().dr_ev_row_capacity(ev.handle) == cap
    assert (ev.pool(), acc.pool()) == (pool, pool_acc)

    assert ev.compact() == 0
    _same_state(_state(ev, acc, keys), after)
    dr.status_check()


@pytest.mark.parametrize("vdt,kdt,dim", [(torch.bfloat16, torch.int64, 8),
                                         (torch.float64, torch.int64, 4),
                                         (torch.float32, torch.int32, 4)])
def test_value_and_key_types(vdt, kdt, dim):
    import deeprec_amd as dr
    rng = np.random.default_rng(dim + (kdt == torch.int32))
    n = 300
    keys = _keys(rng, n, -2**30, 2**30)
    ev = dr.EmbeddingVariable("cmp_types_%s_%s" % (vdt, kdt), dim, 0.5, steps_to_live=2,
                              capacity=1024, device=DEV, key_dtype=kdt, value_dtype=vdt)
    acc = ev.slot("Adagrad", 0.1)
    np_dt = np.float64 if vdt == torch.float64 else np.float32
    dk = _t(keys).to(kdt)
    vers = _versions(n)
    ev.insert(dk, _t(rng.standard_normal((n, dim)).astype(np_dt)), _t(vers))
    acc.insert(dk[::2], _t(rng.standard_normal((keys[::2].size, dim)).astype(np_dt)))
    assert ev.shrink(GS) == 100
    mid = _state(ev, acc, keys)
    assert mid["export"][0].size == 200 and mid["export_acc"][0].size > 50
    assert ev.compact() == 100
    assert ev.rows_allocated() == 200
    after = _state(ev, acc, keys)
    _same_state(after, mid, rows=False)
    want, L, moved = _predict(mid["rows"][vers == KEEP], n)
    assert moved > 10
    np.testing.assert_array_equal(after["rows"][vers == KEEP], want)
    dr.status_check()


def _two_batches(name, evict_first):
    """1000 keys, then 500 more: rows 0..999 and 1000..1499."""
    import deeprec_amd as dr
    rng = np.random.default_rng(77)
    keys = _keys(rng, 1500)
    ev = dr.EmbeddingVariable(name, 4, 0.5, steps_to_live=2, capacity=2048, device=DEV)
    vers = np.full(1500, KEEP, np.int64)
    if evict_first:
        vers[:1000] = EVICT
    else:
        vers[1000:] = EVICT
    vals = rng.standard_normal((1500, 4)).astype(np.float32)
    ev.insert(_t(keys[:1000]), _t(vals[:1000]), _t(vers[:1000]))
    ev.insert(_t(keys[1000:]), _t(vals[1000:]), _t(vers[1000:]))
    rows = ev.find(_t(keys)).cpu().numpy()
    assert sorted(rows[:1000].tolist()) == list(range(1000))
    assert sorted(rows[1000:].tolist()) == list(range(1000, 1500))
    return dr, ev, keys, vers == KEEP


def test_edge_empty_and_no_holes():
    import deeprec_amd as dr
    ev = dr.EmbeddingVariable("cmp_empty", 4, 0.5, steps_to_live=2, capacity=1024, device=DEV)
    assert ev.compact() == 0 and ev.rows_allocated() == 0
    rng = np.random.default_rng(3)
    keys = _keys(rng, 100)
    ev.insert(_t(keys), _t(rng.standard_normal((100, 4)).astype(np.float32)),
              _t(np.full(100, KEEP, np.int64)))
    assert ev.shrink(GS) == 0
    before = _state(ev, None, keys)
    assert ev.compact() == 0 and ev.rows_allocated() == 100
    _same_state(_state(ev, None, keys), before)
    dr.status_check()


def test_edge_every_key_evicted():
    import deeprec_amd as dr
    rng = np.random.default_rng(4)
    keys = _keys(rng, 700)
    ev = dr.EmbeddingVariable("cmp_all", 4, 0.5, steps_to_live=2, capacity=1024, device=DEV)
    ev.track_updates()
    ev.insert(_t(keys), _t(rng.standard_normal((700, 4)).astype(np.float32)),
              _t(np.full(700, EVICT, np.int64)))
    ev.mark_updated(_t(keys))
    assert ev.shrink(GS) == 700
    assert ev.compact() == 700
    assert ev.rows_allocated() == 0 and int(ev.total_count()[0]) == 0
    assert ev.updated_count() == 0 and ev.export()[0].numel() == 0
    # the rows are used again, from 0
    new = _keys(np.random.default_rng(5), 300)
    vals = rng.standard_normal((300, 4)).astype(np.float32)
    ev.insert(_t(new), _t(vals), _t(np.full(300, KEEP, np.int64)))
    assert sorted(ev.find(_t(new)).tolist()) == list(range(300))
    assert ev.key_meta(new)[1].tolist() == [KEEP] * 300
    np.testing.assert_array_equal(ev.sparse_read(_t(new)).cpu().numpy(), vals)
    assert ev.rows_allocated() == 300 == int(ev.total_count()[0])
    assert ev.export_updated()[0].numel() == 0          # no stale bit on the reused rows
    dr.status_check()


def test_edge_holes_only_at_the_tail():
    dr, ev, keys, kept = _two_batches("cmp_tail", evict_first=False)
    assert ev.shrink(GS) == 500
    mid = _state(ev, None, keys)
    assert ev.compact() == 500
    assert ev.rows_allocated() == 1000
    _same_state(_state(ev, None, keys), mid)             # the rows too: nothing moved
    dr.status_check()


def test_edge_every_survivor_moves():
    dr, ev, keys, kept = _two_batches("cmp_head", evict_first=True)
    assert ev.shrink(GS) == 1000
    mid = _state(ev, None, keys)
    assert ev.compact() == 1000
    assert ev.rows_allocated() == 500
    after = _state(ev, None, keys)
    _same_state(after, mid, rows=False)
    want, L, moved = _predict(mid["rows"][kept], 1500)
    assert (L, moved) == (500, 500)
    np.testing.assert_array_equal(after["rows"][kept], want)
    np.testing.assert_array_equal(want, mid["rows"][kept] - 1000)   # order kept: rows 0..499
    dr.status_check()


@pytest.mark.parametrize("n", [300007, 2100003])
def test_edge_more_than_one_scan_tile(n):
    """The rank scan beyond one 8192-word chunk of its one-block form (300007
    rows = 9376 words) and in its tiled form (2100003 rows = 65626 words >
    65536); neither the row count nor the live count is a multiple of 32."""
    import deeprec_amd as dr
    ev = dr.EmbeddingVariable("cmp_big_%d" % n, 2, 0.5, steps_to_live=2, capacity=n, device=DEV)
    keys = torch.arange(n, dtype=torch.int64, device=DEV) * 7 - 3 * n
    vers = torch.full((n,), KEEP, dtype=torch.int64, device=DEV)
    vers[::3] = EVICT
    kept = vers == KEEP
    vals = torch.stack([keys.float(), (keys % 1000).float()], 1)
    ev.insert(keys, vals, vers)
    cap = dr._lib.lib().dr_ev_row_capacity(ev.handle)
    evicted = (n + 2) // 3
    assert ev.shrink(GS) == evicted
    rows = ev.find(keys)
    assert ev.compact() == evicted
    L = n - evicted
    assert n % 32 and L % 32 and ev.rows_allocated() == L == int(ev.total_count()[0])
    want, L2, moved = _predict(rows[kept].cpu().numpy(), n)
    assert L2 == L and moved > 1000
    after = ev.find(keys)
    np.testing.assert_array_equal(after[kept].cpu().numpy(), want)
    assert torch.equal(after[~kept], rows[~kept])
    got = ev.sparse_read(keys, read_only=True)
    assert torch.equal(got[kept], vals[kept])
    assert bool((got[~kept] == 0.5).all())
    assert ev.key_meta(keys[kept][-1000:].cpu().numpy())[1].tolist() == [KEEP] * 1000
    assert dr._lib.lib().dr_ev_row_capacity(ev.handle) == cap
    dr.status_check()


def _counter_ev(dr, name, **kw):
    opt = dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(filter_freq=3))
    return dr.EmbeddingVariable(name, 4, 0.5, steps_to_live=2, capacity=1024, device=DEV,
                                ev_option=opt, **kw)


def test_tail_reset_admission_timeline():
    """A stale freq left in the reclaimed tail would admit a new key early."""
    import deeprec_amd as dr
    rng = np.random.default_rng(6)
    old, new = _keys(rng, 200), _keys(np.random.default_rng(8), 200)
    assert not np.isin(new, old).any()
    ev, twin = _counter_ev(dr, "cmp_adm"), _counter_ev(dr, "cmp_adm_twin")
    sgd = dr.GradientDescentOptimizer(0.1)
    for _ in range(3):
        ev.sparse_read(_t(old))
    ev.pending_grads.append(dr.IndexedSlices(_t(np.ones((200, 4), np.float32)), _t(old)))
    sgd.apply_gradients([ev], global_step=1)
    fr, ve, has = ev.key_meta(old)
    assert (fr >= 3).all() and has.all()
    assert ev.shrink(GS) == 200
    assert ev.compact() == 200 and ev.rows_allocated() == 0
    admitted = []
    for step in range(5):
        a, b = ev.sparse_read(_t(new)), twin.sparse_read(_t(new))
        assert torch.equal(a, b)
        ma, mb = ev.key_meta(new), twin.key_meta(new)
        for x, y in zip(ma, mb):
            np.testing.assert_array_equal(x, y)
        if step == 0:
            assert (ma[0] == 1).all()                    # counted from zero
        fa, fb = (ev.find(_t(new)) >= 0).cpu().numpy(), (twin.find(_t(new)) >= 0).cpu().numpy()
        np.testing.assert_array_equal(fa, fb)
        admitted.append(int(fb.sum()))
        _same(_snap(ev.export()), _snap(twin.export()))
    assert admitted[0] == 0 and admitted[-1] == 200      # the twin's timeline has both ends
    dr.status_check()


def test_tail_reset_updated_count_is_exact():
    import deeprec_amd as dr
    rng = np.random.default_rng(9)
    keys = _keys(rng, 600)
    ev = _counter_ev(dr, "cmp_dirty")
    vers = _versions(600)
    ev.insert(_t(keys), _t(rng.standard_normal((600, 4)).astype(np.float32)), _t(vers),
              _t(np.full(600, 5, np.int64)))
    ev.track_updates()
    marked = keys[::2]
    ev.mark_updated(_t(marked))
    assert ev.shrink(GS) == 200
    upd = _snap(ev.export_updated())
    live_marked = int((vers[::2] == KEEP).sum())
    assert upd[0].size == live_marked < ev.updated_count() == 300
    assert ev.compact() == 200
    assert ev.updated_count() == live_marked
    _same(_snap(ev.export_updated()), upd)
    # marks after the compaction land on the new rows
    ev.clear_updated()
    kept = keys[vers == KEEP]
    ev.mark_updated(_t(kept[:77]))
    got = _snap(ev.export_updated())
    assert ev.updated_count() == 77 == got[0].size
    np.testing.assert_array_equal(got[0], np.sort(kept[:77]))
    dr.status_check()


def test_memory_stays_bounded_under_churn():
    import deeprec_amd as dr
    lib = dr._lib.lib()
    a = dr.EmbeddingVariable("cmp_churn", 4, 0.5, steps_to_live=1, capacity=4096, device=DEV)
    b = dr.EmbeddingVariable("cmp_churn_twin", 4, 0.5, steps_to_live=1, capacity=4096, device=DEV)
    cap0 = lib.dr_ev_row_capacity(a.handle)
    assert cap0 == lib.dr_ev_row_capacity(b.handle) == 4096
    rng = np.random.default_rng(10)
    allkeys = _keys(rng, 600 * 14)
    opt = dr.GradientDescentOptimizer(0.1)
    inserted, rnd = 0, 0
    while inserted <= 2 * cap0:
        k = allkeys[inserted:inserted + 600]
        g = rng.standard_normal((600, 4)).astype(np.float32)
        for ev in (a, b):
            ev.sparse_read(_t(k))
            ev.pending_grads.append(dr.IndexedSlices(_t(g), _t(k)))
            opt.apply_gradients([ev], global_step=rnd)
            assert int(ev.total_count()[0]) <= cap0 // 2     # 3 rounds of keys at the most
            ev.shrink(rnd)
        live = int(a.total_count()[0])
        assert live == int(b.total_count()[0]) == min(rnd + 1, 2) * 600
        a.compact()
        assert a.rows_allocated() <= live
        inserted += 600
        rnd += 1
    assert inserted > 2 * cap0
    assert lib.dr_ev_row_capacity(a.handle) == cap0
    assert lib.dr_ev_row_capacity(b.handle) > cap0 and b.rows_allocated() == inserted
    _same(_snap(a.export()), _snap(b.export()))
    dr.status_check()


@pytest.mark.parametrize("optname", ["GradientDescentOptimizer", "AdagradOptimizer"])
def test_training_is_unaffected(optname, tmp_path):
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    rng = np.random.default_rng(11)
    B, D, F = 256, 8, 2
    batches = [([rng.integers(150 * s, 150 * s + 400, B).astype(np.int64) for _ in range(F)],
                rng.standard_normal((B, F * D)).astype(np.float32)) for s in range(6)]
    ind = np.stack([np.arange(B), np.zeros(B, np.int64)], 1)
    models = []
    for tag, compact in (("c", True), ("p", False)):
        evs = [dr.EmbeddingVariable("cmp_train_%s_%s_%d" % (optname, tag, f), D, 0.05 * (f + 1),
                                    steps_to_live=2, capacity=1024, device=DEV)
               for f in range(F)]
        models.append((tag, compact, evs, getattr(dr, optname)(0.05)))
    (tmp_path / "c").mkdir()
    (tmp_path / "p").mkdir()
    reclaimed = 0
    for step, (ids, g) in enumerate(batches):
        files = []
        for tag, compact, evs, opt in models:
            sps = [dr.SparseTensor(_t(ind), _t(ids[f]), (B, 1)) for f in range(F)]
            out = dr.embedding_lookup_sparse_multi(evs, sps, combiner="sum")
            out.backward(_t(g))
            opt.apply_gradients(evs, global_step=10 + step)
            if step % 2 == 1:
                variables = {}
                for f, ev in enumerate(evs):
                    variables["t%d" % f] = ev
                    for sname, slot in ev._slots.items():
                        variables["t%d/%s" % (f, sname)] = slot
                prefix = str(tmp_path / tag / ("m.ckpt-%d" % step))
                ck.save(prefix, variables, global_step=10 + step, compact=compact)
                files.append([open(p, "rb").read()
                              for p in (ck.data_path(prefix), ck.index_path(prefix))])
                alloc = [ev.rows_allocated() for ev in evs]
                count = [int(ev.total_count()[0]) for ev in evs]
                if compact:
                    assert alloc == count
                else:
                    reclaimed += sum(alloc) - sum(count)
        if files:
            assert files[0] == files[1] and len(files[0][0]) > 1000
    assert reclaimed > 100                       # keys were evicted on the way
    for ea, eb in zip(models[0][2], models[1][2]):
        _same(_snap(ea.export()), _snap(eb.export()))
        for sname in ea._slots:
            _same(_snap(ea._slots[sname].export()), _snap(eb._slots[sname].export()))
    dr.status_check()


def test_refused_inside_stream_capture():
    """The call synchronises, so it is refused while its stream captures --
    before it touches anything -- and works once the capture has ended."""
    import deeprec_amd as dr
    from deeprec_amd._lib import INVALID_ARGUMENT, lib, stream_handle
    ev = dr.EmbeddingVariable("cmp_capture", 4, 0.5, steps_to_live=2, capacity=1024, device=DEV)
    keys = np.arange(100, dtype=np.int64)
    ev.insert(_t(keys), _t(np.ones((100, 4), np.float32)), _t(_versions(100)))
    assert ev.shrink(GS) == 34
    x = torch.zeros(8, device=DEV)
    n = C.c_int64(-5)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x += 1
        rc = lib().dr_ev_compact(ev.handle, C.byref(n), stream_handle(ev.device))
    assert rc == INVALID_ARGUMENT and lib().dr_last_error()
    assert n.value == 0 and ev.rows_allocated() == 100
    g.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 8
    assert ev.compact() == 34 and ev.rows_allocated() == 66
    dr.status_check()


def test_guards():
    import deeprec_amd as dr
    from deeprec_amd._lib import INVALID_ARGUMENT, lib, stream_handle
    ev = dr.EmbeddingVariable("cmp_guard", 4, 0.5, steps_to_live=2, capacity=1024, device=DEV)
    acc = ev.slot("Adagrad", 0.1)
    keys = np.arange(10, dtype=np.int64)
    ev.sparse_read(_t(keys))
    sl = dr.IndexedSlices(_t(np.ones((10, 4), np.float32)), _t(keys))
    ev.pending_grads.append(sl)
    with pytest.raises(dr.InvalidArgumentError):
        ev.compact()
    with pytest.raises(dr.InvalidArgumentError):
        acc.compact()                               # the key space's primary is checked
    ev.pending_grads.clear()
    acc.pending_grads.append(sl)
    with pytest.raises(dr.InvalidArgumentError):
        ev.compact()
    acc.pending_grads.clear()
    assert acc.compact() == 0                       # through the primary
    n = C.c_int64(-5)
    assert lib().dr_ev_compact(acc.handle, C.byref(n), stream_handle(ev.device)) == INVALID_ARGUMENT
    assert lib().dr_last_error()
    assert lib().dr_ev_rows_allocated(acc.handle, C.byref(n), stream_handle(ev.device)) == 0
    assert n.value == 10 == acc.rows_allocated()
