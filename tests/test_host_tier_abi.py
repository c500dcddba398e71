"""CPU-side checks of the HBM + host-DRAM tier: every new
entry resolves through ctypes with the signature of the Python mirror, the
header declares it, a null EV or tier is DR_INVALID_ARGUMENT with the outputs
untouched and no device touched, the ABI version stays, the Python surface
exists and the pinned signatures around it keep their parameter lists."""
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
    "dr_ev_missing_keys": (I32, [P, I32, P, P, P, P, P, P, P]),
    "dr_ev_demote_to": (I32, [P, I64, I32, P, P, I32, P, P, P, I64, P, P]),
    "dr_ev_promote": (I32, [P, P, I64, P, I32, P, P, P, P]),
    "dr_host_tier_create": (I32, [I32, P, I64, P]),
    "dr_host_tier_destroy": (I32, [P]),
    "dr_host_tier_size": (I32, [P, P]),
    "dr_host_tier_put": (I32, [P, P, I64, P, P, P, P]),
    "dr_host_tier_take": (I32, [P, P, I64, I32, P, P, P, P, P, P]),
    "dr_host_tier_remove": (I32, [P, P, I64, P]),
    "dr_host_tier_shrink": (I32, [P, I64, I64, P]),
    "dr_host_tier_export": (I32, [P, P, P, P, P, P, I64, P]),
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
    assert "typedef struct dr_host_tier dr_host_tier;" in text


def test_null_ev_is_invalid_argument(lib):
    m = C.c_int64(7)
    koff = (C.c_int64 * 2)(0, 4)
    one = (C.c_void_p * 1)(None)
    assert lib.dr_ev_missing_keys(None, 1, None, koff, None, None, None, None,
                                  None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert lib.dr_ev_missing_keys(one, 1, None, koff, None, None, None, None,
                                  None) == INVALID_ARGUMENT      # a null EV in the group
    for policy in (0, 1, 7):
        for max_keys in (-1, 0, 10):
            assert lib.dr_ev_demote_to(None, max_keys, policy, None, None, 0, None, None, None, 0,
                                       C.byref(m), None) == INVALID_ARGUMENT
    assert lib.dr_ev_promote(None, None, 3, None, 0, None, None, None, None) == INVALID_ARGUMENT
    assert m.value == 7      # nothing was written


def test_null_tier_is_invalid_argument(lib):
    n = C.c_int64(7)
    keys = (C.c_int64 * 2)(1, 2)
    assert lib.dr_host_tier_size(None, C.byref(n)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_put(None, keys, 2, None, None, None, None) == INVALID_ARGUMENT
    assert lib.dr_host_tier_take(None, keys, 2, 1, None, None, None, None, None,
                                 C.byref(n)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_remove(None, keys, 2, C.byref(n)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_shrink(None, 5, 1, C.byref(n)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_export(None, None, None, None, None, None, 0,
                                   C.byref(n)) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert n.value == 7
    t = C.c_void_p(11)
    cb = (C.c_int64 * 1)(4)
    assert lib.dr_host_tier_create(0, cb, 1, C.byref(t)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_create(1, None, 1, C.byref(t)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_create(1, cb, 1, None) == INVALID_ARGUMENT
    assert t.value == 11


def test_export_capacity_is_checked(lib):
    t = C.c_void_p()
    cb = (C.c_int64 * 1)(4)
    assert lib.dr_host_tier_create(1, cb, 1, C.byref(t)) == 0
    keys = (C.c_int64 * 3)(5, -1, 0)
    assert lib.dr_host_tier_put(t, keys, 3, None, None, None, None) == 0
    m = C.c_int64(0)
    assert lib.dr_host_tier_export(t, None, None, None, None, None, 0, C.byref(m)) == 0
    assert m.value == 3                                     # null outputs query the count
    out = (C.c_int64 * 3)(9, 9, 9)
    assert lib.dr_host_tier_export(t, out, None, None, None, None, 2,
                                   C.byref(m)) == INVALID_ARGUMENT
    assert list(out) == [9, 9, 9]
    assert lib.dr_host_tier_export(t, out, None, None, None, None, 3, C.byref(m)) == 0
    assert list(out) == [-1, 0, 5]
    assert lib.dr_host_tier_destroy(t) == 0


def test_python_surface_exists():
    import deeprec_amd as dr
    assert dr.StorageType.HBM != dr.StorageType.HBM_DRAM
    assert dr.StorageOption().storage_type == dr.StorageType.HBM
    assert dr.StorageOption(dr.StorageType.HBM_DRAM).storage_type == dr.StorageType.HBM_DRAM
    with pytest.raises(ValueError):
        dr.StorageOption("SSD")
    p = inspect.signature(dr.EmbeddingVariableOption.__init__).parameters
    assert list(p) == ["self", "ht_type", "ht_partition_num", "evict_option", "filter_option",
                       "storage_option"]
    assert p["storage_option"].default is None
    o = dr.EmbeddingVariableOption(storage_option=dr.StorageOption(dr.StorageType.HBM_DRAM))
    assert o.storage_option.storage_type == dr.StorageType.HBM_DRAM
    p = inspect.signature(dr.EmbeddingVariable.demote_to).parameters
    assert list(p) == ["self", "max_keys", "policy", "compact"]
    assert (p["max_keys"].default, p["policy"].default, p["compact"].default) == (None, None, True)
    assert list(inspect.signature(dr.EmbeddingVariable.promote).parameters) == ["self", "keys"]
    assert list(inspect.signature(dr.EmbeddingVariable.tier_count).parameters) == ["self"]
    assert isinstance(dr.EmbeddingVariable.tiered, property)
    for name in ("total_count", "find", "key_meta", "rows_allocated", "shrink_to"):
        assert "HBM" in getattr(dr.EmbeddingVariable, name).__doc__, name


def test_pinned_signatures_stay():
    """tests/test_budget_abi.py::test_pinned_signatures_stay, restated."""
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
    p = inspect.signature(dr.KeyBudgetEvict.__init__).parameters
    assert list(p) == ["self", "max_keys", "policy", "steps_to_live"]
