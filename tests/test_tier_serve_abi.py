"""CPU-side checks of serving pooled read-only lookups from the host-DRAM tier
(DESIGN section 19): the two overlay entries resolve through ctypes with the
signatures of the Python mirror, the header declares them with as many
parameters, null arguments are DR_INVALID_ARGUMENT before any device is
touched, the ABI version stays, and read_only_lookups(serve_tier=...) is
keyword-only, off by default, inherited by nested blocks and per thread."""
import ctypes as C
import inspect
import os
import re
import subprocess
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
ENTRIES = {
    "dr_ev_overlay_resolve": (I32, [P, P, P, I32, P, P, P, P]),
    "dr_ev_overlay_patch_onehot": (I32, [P, P, I64, P, I32, P, P, P, I64, P, I64, I64, I32, I32,
                                         P]),
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


def test_header_declares_the_entries_with_as_many_parameters():
    with open(os.path.join(ROOT, "include", "deeprec_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, (_, args) in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(args), (name, m.group(1))


def test_null_arguments_are_invalid_argument(lib):
    k = (C.c_int64 * 4)(1, 2, 3, 4)
    off = (C.c_int64 * 2)(0, 4)
    kp, op = C.cast(k, P), C.cast(off, P)
    # (host arrays stand in for device pointers: a refused call touches none of them)
    good = [kp, op, None, 1, kp, op, kp, None]
    for i in (0, 1, 4, 5, 6):
        a = list(good)
        a[i] = None
        assert lib.dr_ev_overlay_resolve(*a) == INVALID_ARGUMENT, i
        assert lib.dr_last_error()
    assert lib.dr_ev_overlay_resolve(kp, op, None, 0, kp, op, kp, None) == INVALID_ARGUMENT
    good = [kp, kp, 4, op, 1, kp, op, kp, 4, kp, 4, 4, 0, 0, None]
    for i in (0, 1, 3, 5, 6, 7, 9):
        a = list(good)
        a[i] = None
        assert lib.dr_ev_overlay_patch_onehot(*a) == INVALID_ARGUMENT, i
        assert lib.dr_last_error()
    # every pointer null, and shapes the fused route never has
    assert lib.dr_ev_overlay_patch_onehot(None, None, 0, None, 1, None, None, None, 4, None, 4, 4,
                                          0, 0, None) == INVALID_ARGUMENT
    for words, dim, order, flags in ((6, 6, 0, 0), (4, 16, 0, 0), (4, 4, 7, 0), (4, 4, 0, 1 << 9)):
        a = list(good)
        a[8], a[11], a[12], a[13] = words, dim, order, flags
        a[10] = dim
        assert lib.dr_ev_overlay_patch_onehot(*a) == INVALID_ARGUMENT, (words, dim, order, flags)
    assert list(k) == [1, 2, 3, 4]      # nothing was written


def test_serve_tier_is_keyword_only_and_off_by_default():
    import deeprec_amd as dr
    p = inspect.signature(dr.read_only_lookups.__init__).parameters
    assert list(p) == ["self", "serve_tier"]
    assert p["serve_tier"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["serve_tier"].default is False
    with pytest.raises(TypeError):
        dr.read_only_lookups(True)


def test_flag_nesting_and_threads():
    import deeprec_amd as dr
    from deeprec_amd.kv_variable_ops import read_only_active, read_only_serves_tier
    assert dr.read_only_serves_tier is read_only_serves_tier
    assert not read_only_serves_tier()
    with dr.read_only_lookups():
        assert read_only_active() and not read_only_serves_tier()
        with dr.read_only_lookups(serve_tier=True):
            assert read_only_serves_tier()
        assert read_only_active() and not read_only_serves_tier()    # the inner block's alone
    seen = {}

    def other():
        seen["outside"] = read_only_serves_tier()
        with dr.read_only_lookups():
            seen["plain"] = read_only_serves_tier()

    with dr.read_only_lookups(serve_tier=True) as ctx:
        assert read_only_serves_tier()
        with dr.read_only_lookups():
            assert read_only_serves_tier()          # inherited
            with dr.read_only_lookups(serve_tier=False):
                assert read_only_serves_tier()      # ... however deep
        assert read_only_serves_tier()
        th = threading.Thread(target=other)
        th.start()
        th.join()
        with ctx:                                   # the same object, re-entered
            assert read_only_serves_tier()
        assert read_only_serves_tier()
    assert seen == {"outside": False, "plain": False}
    assert not read_only_serves_tier() and not read_only_active()
    try:
        with dr.read_only_lookups(serve_tier=True):
            raise KeyError("x")
    except KeyError:
        pass
    assert not read_only_serves_tier() and not read_only_active()
