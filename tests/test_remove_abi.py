"""CPU-side checks of keyed removal and the removal log (dr_ev_remove,
dr_ev_track_removals, dr_ev_tracking_removals, dr_ev_removed_count,
dr_ev_export_removed, dr_ev_clear_removed): they resolve through ctypes with
the signatures of the Python mirror, refuse a null EV with
DR_INVALID_ARGUMENT before touching a device, the ABI version stays, and the
Python surface exists."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
ENTRIES = {
    "dr_ev_remove": (I32, [P, P, I64, P, P]),
    "dr_ev_track_removals": (I32, [P, I32, P]),
    "dr_ev_tracking_removals": (I32, [P]),
    "dr_ev_removed_count": (I32, [P, P, P]),
    "dr_ev_export_removed": (I32, [P, P, I64, P, P]),
    "dr_ev_clear_removed": (I32, [P, P]),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "deeprec-1_amd")])
    import deeprec_amd._lib as L
    lib = C.CDLL(LIB)
    for name in tuple(ENTRIES) + ("dr_last_error", "dr_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def test_entries_resolve_and_abi_version_stays(lib):
    import deeprec_amd._lib as L
    for name, sig in ENTRIES.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == sig, name
    assert lib.dr_abi_version() == 2


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "deeprec_amd.h")) as f:
        text = f.read()
    for name in ENTRIES:
        assert name + "(" in text, name


def test_null_ev_is_invalid_argument(lib):
    n = C.c_int64(7)
    keys = (C.c_int64 * 4)(1, 2, 3, 4)
    assert lib.dr_ev_remove(None, keys, 4, C.byref(n), None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert lib.dr_ev_remove(None, None, 0, None, None) == INVALID_ARGUMENT
    assert lib.dr_ev_track_removals(None, 1, None) == INVALID_ARGUMENT
    assert lib.dr_ev_track_removals(None, 0, None) == INVALID_ARGUMENT
    assert lib.dr_ev_tracking_removals(None) == -1
    assert lib.dr_ev_removed_count(None, C.byref(n), None) == INVALID_ARGUMENT
    assert lib.dr_ev_export_removed(None, keys, 4, C.byref(n), None) == INVALID_ARGUMENT
    assert lib.dr_ev_clear_removed(None, None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert n.value == 7      # nothing was written


def test_python_surface_exists():
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    for name in ("remove", "track_removals", "tracking_removals", "removed_count",
                 "export_removed", "clear_removed"):
        assert callable(getattr(dr.EmbeddingVariable, name)), name
    assert list(inspect.signature(dr.EmbeddingVariable.remove).parameters) == ["self", "keys"]
    assert inspect.signature(dr.EmbeddingVariable.track_removals).parameters["on"].default is True
    p = inspect.signature(ck.restore_incremental).parameters
    assert list(p) == ["prefix", "variables", "partition_id", "partition_num", "compact"]
    assert p["compact"].default is False
    assert list(inspect.signature(ck.save_incremental).parameters) == ["prefix", "variables",
                                                                       "global_step"]
