"""CPU-side checks of the incremental-checkpoint entries (update tracking,
delta export, upsert): the C entries resolve through ctypes with the
signatures of the Python mirror, each refuses null arguments with
DR_INVALID_ARGUMENT before it touches a device, the Python surface exists, and
the bundle writer round-trips a delta's five tensors under the
NAME-sparse_incr_* names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

ENTRIES = ("dr_ev_track_updates", "dr_ev_tracking_updates", "dr_ev_mark_updated",
           "dr_ev_updated_count", "dr_ev_export_updated", "dr_ev_clear_updated", "dr_ev_upsert")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "deeprec-1_amd")])
    import deeprec_amd._lib as L
    lib = C.CDLL(LIB)
    for name in ENTRIES + ("dr_last_error", "dr_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def test_entries_resolve_and_abi_version_stays(lib):
    import deeprec_amd._lib as L
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert lib.dr_abi_version() == 2


def test_null_arguments_are_invalid_argument(lib):
    m = C.c_int64(0)
    keys = (C.c_int64 * 4)(1, 2, 3, 4)
    koff = (C.c_int64 * 3)(0, 2, 4)
    assert lib.dr_ev_track_updates(None, 1, None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert lib.dr_ev_tracking_updates(None) == -1
    assert lib.dr_ev_updated_count(None, C.byref(m), None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert lib.dr_ev_export_updated(None, None, None, None, None, 0, C.byref(m),
                                    None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert lib.dr_ev_clear_updated(None, None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert lib.dr_ev_upsert(None, keys, 4, keys, None, None, 0, 0, None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    # the grouped mark: a null table list, null tables, a bad table count
    assert lib.dr_ev_mark_updated(None, 1, keys, koff, None, None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    evs = (C.c_void_p * 2)(None, None)
    assert lib.dr_ev_mark_updated(evs, 2, keys, koff, None, None) == INVALID_ARGUMENT
    assert lib.dr_ev_mark_updated(evs, 0, keys, koff, None, None) == INVALID_ARGUMENT
    assert lib.dr_ev_mark_updated(evs, 2, None, koff, None, None) == INVALID_ARGUMENT


def test_python_surface_exists():
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    for name in ("track_updates", "mark_updated", "updated_count", "export_updated",
                 "clear_updated", "upsert"):
        assert callable(getattr(dr.EmbeddingVariable, name)), name
    assert callable(ck.save_incremental) and callable(ck.restore_incremental)
    assert callable(dr.AdagradOptimizer._record_updates)


def test_incremental_tensor_names_round_trip(tmp_path):
    from deeprec_amd import checkpoint as ck
    assert ck.INCR_SUFFIX == "sparse_incr_"
    rng = np.random.default_rng(5)
    offs = np.zeros(1001, np.int32)
    offs[8:] = 3
    keys = np.array([7, 1007, 2007], np.int64)
    vals = rng.standard_normal((3, 6)).astype(np.float32)
    vers = np.array([4, 5, 6], np.int64)
    frqs = np.zeros(0, np.int64)
    pre = str(tmp_path / "delta")
    w = ck.BundleWriter(pre)
    ck.write_ev_tensors(w, "emb/part_0", offs, keys, vals, vers, frqs, ck.INCR_SUFFIX)
    ck.write_ev_tensors(w, "emb/part_0", offs, keys[:0], vals[:0], vers[:0], frqs)
    w.finish()
    r = ck.BundleReader(pre)
    incr = ["emb/part_0-sparse_incr_" + t
            for t in ("freqs", "keys", "partition_offset", "values", "versions")]
    full = ["emb/part_0-" + t for t in ("freqs", "keys", "partition_offset", "values", "versions")]
    assert r.keys() == sorted(incr + full)
    np.testing.assert_array_equal(r.lookup("emb/part_0-sparse_incr_partition_offset"), offs)
    np.testing.assert_array_equal(r.lookup("emb/part_0-sparse_incr_keys"), keys)
    np.testing.assert_array_equal(r.lookup("emb/part_0-sparse_incr_values"), vals)
    np.testing.assert_array_equal(r.lookup("emb/part_0-sparse_incr_versions"), vers)
    assert r.dtype_and_shape("emb/part_0-sparse_incr_freqs") == (np.dtype(np.int64), (0,))
    assert r.dtype_and_shape("emb/part_0-keys")[1] == (0,)
