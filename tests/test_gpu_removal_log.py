"""The removal log of an EmbeddingVariable's key space (dr_ev_track_removals):
while it is on, shrink() and remove() append every key they drop, and
export_removed() gives the distinct logged keys in ascending order.

The reference is the ascending set difference of export() keys before and
after the call.  The global-step timeline is test_gpu_shrink.py's
(steps_to_live 5, id 2 * i trained at step i for i < 10, shrink at step 10),
restated here; the L2 form uses that file's rows and threshold.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _keys_of(ev):
    return ev.export()[0].cpu().numpy()


def _snap(ev):
    k, v, ve, fr = ev.export()
    return (k.cpu().numpy(), v.cpu().numpy().view(np.uint32), ve.cpu().numpy(), fr.cpu().numpy())


def _removed(ev):
    return ev.export_removed().cpu().numpy()


def _log_init():
    """First size of the log buffer, from the implementation."""
    with open(os.path.join(ROOT, "deeprec-1_amd", "csrc", "ev.hip")) as f:
        m = re.search(r"kRmLogInit\s*=\s*(\d+)\s*;", f.read())
    return int(m.group(1))


def test_shrink_by_global_step_is_logged():
    import deeprec_amd as dr
    ev = dr.EmbeddingVariable("rlog_gs", 3, 1.0, steps_to_live=5, device=DEV)
    opt = dr.GradientDescentOptimizer(0.1)
    for i in range(10):
        ev.sparse_read(_t(np.array([2 * i], np.int64)))
        ev.pending_grads.append(dr.IndexedSlices(_t(np.full((1, 3), 2.0, np.float32)),
                                                 _t(np.array([2 * i], np.int64))))
        opt.apply_gradients([ev], global_step=i)
    assert not ev.tracking_removals()
    ev.track_removals()
    assert ev.tracking_removals() and ev.removed_count() == 0 and _removed(ev).size == 0
    before = _keys_of(ev)
    assert ev.shrink(10) == 5                       # 10 - i > 5  <=>  i < 5
    after = _keys_of(ev)
    want = np.setdiff1d(before, after)
    assert want.tolist() == [0, 2, 4, 6, 8]
    assert ev.removed_count() == 5
    got = _removed(ev)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_removed(ev), want)          # the export leaves the log
    assert ev.shrink(10) == 0 and ev.removed_count() == 5      # nothing more to drop
    ev.track_removals(False)
    assert not ev.tracking_removals()
    with pytest.raises(dr.InvalidArgumentError):
        ev.removed_count()
    ev.track_removals()
    assert ev.removed_count() == 0                  # on again: an empty log
    dr.status_check()


def test_shrink_by_l2_weight_is_logged():
    import deeprec_amd as dr
    rng = np.random.default_rng(5)
    n, D, thr = 500, 8, 1.5
    rows = (rng.standard_normal((n, D)) * 0.6).astype(np.float32)
    ev = dr.EmbeddingVariable("rlog_l2", D, 0.0, l2_weight_threshold=thr, device=DEV)
    acc = ev.slot("Adagrad", 0.1)
    ev.insert(_t(np.arange(n, dtype=np.int64) * 7), _t(rows))
    acc.track_removals()                            # the log belongs to the key space
    assert ev.tracking_removals()
    before = _keys_of(ev)
    removed = ev.shrink()
    want = np.setdiff1d(before, _keys_of(ev))
    assert removed == want.size and 50 < removed < n - 50
    np.testing.assert_array_equal(_removed(ev), want)
    np.testing.assert_array_equal(_removed(acc), want)
    dr.status_check()


def test_remove_logs_twice_evicted_once_exported_and_minus_one():
    import deeprec_amd as dr
    keys = np.array([-1, 0, 3, 11, -40, 2**40], np.int64)
    ev = dr.EmbeddingVariable("rlog_rm", 4, 0.5, steps_to_live=2, capacity=512, device=DEV)
    ev.insert(_t(keys), _t(np.ones((6, 4), np.float32)), _t(np.array([0, 9, 9, 9, 0, 9], np.int64)))
    ev.track_removals()
    assert ev.remove(_t(np.array([11, 12345], np.int64))) == 1         # remove() logs
    np.testing.assert_array_equal(_removed(ev), [11])
    assert ev.shrink(10) == 2                                          # -1 and -40 (10 - 0 > 2)
    np.testing.assert_array_equal(_removed(ev), [-40, -1, 11])         # ascending as signed
    ev.sparse_read(_t(np.array([11, -1], np.int64)))                   # re-created ...
    assert ev.remove(_t(np.array([11, -1, 3], np.int64))) == 3         # ... and evicted again
    assert ev.removed_count() == 6
    np.testing.assert_array_equal(_removed(ev), [-40, -1, 3, 11])
    # the log is not filtered against the map: 3 is live again and stays logged
    ev.sparse_read(_t(np.array([3], np.int64)))
    np.testing.assert_array_equal(_removed(ev), [-40, -1, 3, 11])
    assert _keys_of(ev).tolist() == [0, 3, 2**40]
    ev.clear_removed()
    assert ev.removed_count() == 0 and _removed(ev).size == 0
    assert ev.tracking_removals()
    assert ev.remove(_t(np.array([0], np.int64))) == 1                 # the cleared log goes on
    np.testing.assert_array_equal(_removed(ev), [0])
    dr.status_check()


def _groups(sizes, seed):
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    keys = np.unique(rng.integers(-2**62, 2**62, 2 * n).astype(np.int64))
    keys = keys[keys != -1]
    rng.shuffle(keys)
    keys = keys[:n]
    grp = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    return keys, grp, rng.standard_normal((n, 4)).astype(np.float32)


def test_log_grows_and_log_off_twin_agrees():
    """A few thousand evictions in four shrinks carry the log across three
    doublings of its buffer, one per shrink after the first; a twin with the
    log off evicts the same keys."""
    import deeprec_amd as dr
    init = _log_init()
    cum = [init * 5 // 8, init * 15 // 8, init * 15 // 4, init * 19 // 4]
    assert cum[0] <= init < cum[1] <= 2 * init < cum[2] <= 4 * init < cum[3] <= 8 * init
    sizes = [cum[0]] + [b - a for a, b in zip(cum, cum[1:])] + [400]
    keys, grp, vals = _groups(sizes, 21)
    vers = np.array([0, 10, 20, 30, 100], np.int64)[grp]
    evs = []
    for tag in ("on", "off"):
        ev = dr.EmbeddingVariable("rlog_grow_" + tag, 4, 0.5, steps_to_live=2, capacity=8192,
                                  device=DEV)
        ev.insert(_t(keys), _t(vals), _t(vers))
        evs.append(ev)
    on, off = evs
    on.track_removals()
    logged = 0
    for g, gs in enumerate((3, 13, 23, 33)):                      # gs - version > 2 group by group
        before = _keys_of(on)
        n_on, n_off = on.shrink(gs), off.shrink(gs)
        assert n_on == n_off == sizes[g]
        for a, b in zip(_snap(on), _snap(off)):
            np.testing.assert_array_equal(a, b)
        logged += n_on
        assert on.removed_count() == logged
        np.testing.assert_array_equal(_removed(on), np.sort(keys[grp <= g]))
        np.testing.assert_array_equal(np.setdiff1d(before, _keys_of(on)), np.sort(keys[grp == g]))
    assert int(on.total_count()[0]) == int(off.total_count()[0]) == 400
    assert on.compact() == off.compact() == logged
    dr.status_check()


def test_export_capacity_too_small():
    import deeprec_amd as dr
    from deeprec_amd._lib import INVALID_ARGUMENT, lib, stream_handle
    ev = dr.EmbeddingVariable("rlog_cap", 4, 0.5, capacity=512, device=DEV)
    keys = np.arange(50, dtype=np.int64)
    ev.sparse_read(_t(keys))
    ev.track_removals()
    assert ev.remove(_t(keys[:20])) == 20
    ev.sparse_read(_t(keys[:5]))
    assert ev.remove(_t(keys[:5])) == 5             # 25 entries, 20 distinct keys
    st = stream_handle(ev.device)
    m = C.c_int64(-3)
    assert lib().dr_ev_export_removed(ev.handle, None, 0, C.byref(m), st) == 0
    assert m.value == 20 and ev.removed_count() == 25
    out = torch.full((32,), -7, dtype=torch.int64, device=DEV)
    m = C.c_int64(-3)
    assert lib().dr_ev_export_removed(ev.handle, out.data_ptr(), 19, C.byref(m),
                                      st) == INVALID_ARGUMENT
    assert lib().dr_last_error() and m.value == 20
    assert out.tolist() == [-7] * 32                # nothing was written
    assert lib().dr_ev_export_removed(ev.handle, out.data_ptr(), 20, C.byref(m), st) == 0
    assert m.value == 20 and out.tolist() == list(range(20)) + [-7] * 12
    dr.status_check()
