"""CPU-side checks of the mark-by-row entry of the incremental checkpoints
(dr_ev_mark_updated_rows): it resolves through ctypes with the signature of the
Python mirror, the ABI version stays, every argument check refuses with
DR_INVALID_ARGUMENT before any device work, and the Python surface exists.

The argument checks run before the entry reads an EV, so a table that must be
non-null here is the address of a zeroed buffer: each call below fails a check
first, and the error text says which one."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3
ENTRY = "dr_ev_mark_updated_rows"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "deeprec-1_amd")])
    import deeprec_amd._lib as L
    lib = C.CDLL(LIB)
    for name in (ENTRY, "dr_last_error", "dr_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def test_entry_resolves_and_abi_version_stays(lib):
    import deeprec_amd._lib as L
    assert hasattr(lib, ENTRY)
    assert ENTRY in L.SIGNATURES
    assert len(L.SIGNATURES[ENTRY][1]) == 7
    assert lib.dr_abi_version() == 2


def _refused(lib, what, *args):
    assert lib.dr_ev_mark_updated_rows(*args) == INVALID_ARGUMENT
    msg = lib.dr_last_error()
    assert msg and what in msg.decode(), (what, msg)


def test_argument_checks_are_invalid_argument(lib):
    import deeprec_amd._lib as L
    rows = (C.c_int64 * 6)(0, 1, 2, 3, 4, 5)
    fake = C.create_string_buffer(64)           # never read: every call fails a check first
    ev = C.addressof(fake)
    evs = (C.c_void_p * 3)(ev, None, ev)
    koff = (C.c_int64 * 4)(0, 2, 4, 6)
    big = (C.c_void_p * (L.MAX_GROUP + 1))(*([ev] * (L.MAX_GROUP + 1)))
    kbig = (C.c_int64 * (L.MAX_GROUP + 2))()
    nd = (C.c_void_p * 3)(None, None, None)
    # a null table list, a null koff, T outside 1..DR_MAX_GROUP
    _refused(lib, "bad argument", None, 3, rows, koff, 0, None, None)
    _refused(lib, "bad argument", evs, 3, rows, None, 0, None, None)
    _refused(lib, "bad argument", evs, 0, rows, koff, 0, None, None)
    _refused(lib, "bad argument", evs, -1, rows, koff, 0, None, None)
    _refused(lib, "bad argument", big, L.MAX_GROUP + 1, rows, kbig, 0, None, None)
    # every table null
    _refused(lib, "every ev is null", (C.c_void_p * 3)(None, None, None), 3, rows, koff, 0, None,
             None)
    # null rows with a non-zero total
    _refused(lib, "null rowsel", evs, 3, None, koff, 0, None, None)
    # koff decreasing, koff negative
    _refused(lib, "koff", evs, 3, rows, (C.c_int64 * 4)(0, 4, 2, 6), 0, None, None)
    _refused(lib, "koff", evs, 3, rows, (C.c_int64 * 4)(-2, 0, 2, 4), 0, None, None)
    # record-major rows: koff[t] == t * koff[1], and no per-table device counts
    _refused(lib, "record-major", evs, 3, rows, (C.c_int64 * 4)(0, 2, 4, 5), 1, None, None)
    _refused(lib, "record-major", evs, 3, rows, (C.c_int64 * 4)(1, 2, 4, 6), 1, None, None)
    _refused(lib, "record-major", evs, 3, rows, koff, 1, nd, None)


def test_python_surface_exists():
    import deeprec_amd as dr
    from deeprec_amd import embedding_ops as eo
    from deeprec_amd import kv_variable_ops as kv
    for name in ("mark_updated_rows", "tracking_by_row", "track_updates", "tracking_updates"):
        assert callable(getattr(dr.EmbeddingVariable, name)), name
    assert callable(kv.mark_updated_rows_grouped)
    assert callable(eo._RowsPending.mark_rows)
    sig = inspect.signature(dr.EmbeddingVariable.track_updates)
    assert sig.parameters["by_row"].default is False
    assert sig.parameters["on"].default is True
