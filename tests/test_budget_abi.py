"""CPU-side checks of the key budget (dr_ev_shrink_to): the entry resolves
through ctypes with the signature of the Python mirror, the header declares it
and both policy macros, it refuses a null EV with DR_INVALID_ARGUMENT before
touching a device, the ABI version stays, and the Python surface exists while
the pinned signatures around it keep their parameter lists."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
ENTRIES = {
    "dr_ev_shrink_to": (I32, [P, I64, I32, P, P]),
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


def test_entry_resolves_and_abi_version_stays(lib):
    import deeprec_amd._lib as L
    for name, sig in ENTRIES.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == sig, name
    assert lib.dr_abi_version() == 2


def test_header_declares_the_entry_and_the_policies():
    with open(os.path.join(ROOT, "include", "deeprec_amd.h")) as f:
        text = f.read()
    for name in ENTRIES:
        assert name + "(" in text, name
    assert re.search(r"^#define\s+DR_EVICT_LRU\s+0\b", text, re.M)
    assert re.search(r"^#define\s+DR_EVICT_LFU\s+1\b", text, re.M)


def test_null_ev_is_invalid_argument(lib):
    n = C.c_int64(7)
    for policy in (0, 1, 7):
        for max_keys in (-1, 0, 10):
            assert lib.dr_ev_shrink_to(None, max_keys, policy, C.byref(n), None) == INVALID_ARGUMENT
            assert lib.dr_last_error()
    assert lib.dr_ev_shrink_to(None, 10, 0, None, None) == INVALID_ARGUMENT
    assert n.value == 7      # nothing was written


def test_python_surface_exists():
    import deeprec_amd as dr
    p = inspect.signature(dr.EmbeddingVariable.shrink_to).parameters
    assert list(p) == ["self", "max_keys", "policy"]
    assert p["max_keys"].default is inspect.Parameter.empty and p["policy"].default == "lru"
    p = inspect.signature(dr.KeyBudgetEvict.__init__).parameters
    assert list(p) == ["self", "max_keys", "policy", "steps_to_live"]
    assert p["policy"].default == "lru" and p["steps_to_live"].default is None
    o = dr.KeyBudgetEvict(300, "lfu", steps_to_live=9)
    assert (o.max_keys, o.policy, o.steps_to_live) == (300, "lfu", 9)
    with pytest.raises(ValueError):
        dr.KeyBudgetEvict(300, "fifo")
    assert dr.GlobalStepEvict(4).steps_to_live == 4
    assert not hasattr(dr.GlobalStepEvict(4), "max_keys")


def test_pinned_signatures_stay():
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    assert list(inspect.signature(ck.save).parameters) == ["prefix", "variables", "global_step",
                                                           "compact"]
    assert list(inspect.signature(ck.save_incremental).parameters) == ["prefix", "variables",
                                                                       "global_step"]
    assert list(inspect.signature(ck.restore_incremental).parameters) == [
        "prefix", "variables", "partition_id", "partition_num", "compact"]
    assert list(inspect.signature(dr.EmbeddingVariable.__init__).parameters) == [
        "self", "name", "embedding_dim", "initializer", "steps_to_live", "ev_option", "capacity",
        "device", "_primary", "_slot_index", "l2_weight_threshold", "key_dtype", "value_dtype"]
    assert "global_step is given" in ck.save_incremental.__doc__    # the budget's difference
