"""CPU-side checks of incremental checkpoints for a tiered key space (DESIGN
section 17): the new entries resolve through ctypes with the signature of the
Python mirror, the header declares them with as many parameters, a null EV is
DR_INVALID_ARGUMENT with no device touched, the ABI version stays, and the
opt-in exists on StorageOption with its default off."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

P, I32, I64, U32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
ENTRIES = {
    "dr_ev_log_removed": (I32, [P, P, I64, P]),
    "dr_host_tier_count_masked": (I32, [P, U32, P]),
    "dr_host_tier_export_masked": (I32, [P, U32, P, P, P, P, P, I64, P]),
    "dr_host_tier_clear_bits": (I32, [P, U32, P]),
    "dr_host_tier_or_bits": (I32, [P, P, I64, U32, U32, P]),
    "dr_host_tier_shrink_keys": (I32, [P, I64, I64, P, I64, P]),
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
    assert lib.dr_abi_version() == 2                        # additive: no version step
    assert L.TIER_UPDATED == 1 << 16


def test_header_declares_the_entries_with_matching_argument_counts():
    with open(os.path.join(ROOT, "include", "deeprec_amd.h")) as f:
        text = f.read()
    assert re.search(r"#define\s+DR_TIER_UPDATED\s+\(1u << 16\)", text)
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)       # (a comment may hold a comma)
    for name, (_, args) in ENTRIES.items():
        m = re.search(r"\bint\s+%s\(([^)]*)\);" % name, bare)
        assert m, name
        assert len(m.group(1).split(",")) == len(args), (name, m.group(1))


def test_log_removed_refuses_a_null_ev_without_a_device(lib):
    keys = (C.c_int64 * 2)(1, 2)
    assert lib.dr_ev_log_removed(None, keys, 2, None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    assert lib.dr_ev_log_removed(None, None, 0, None) == INVALID_ARGUMENT


def test_storage_option_opt_in():
    import deeprec_amd as dr
    assert dr.StorageOption(dr.StorageType.HBM_DRAM).incremental is False
    assert dr.StorageOption().incremental is False
    assert dr.StorageOption(dr.StorageType.HBM_DRAM, incremental=True).incremental is True
    assert dr.StorageOption(dr.StorageType.HBM_DRAM, True).storage_type == dr.StorageType.HBM_DRAM
    with pytest.raises(ValueError):
        dr.StorageOption(dr.StorageType.HBM, incremental=True)
    with pytest.raises(ValueError):
        dr.StorageOption(incremental=True)
    p = inspect.signature(dr.StorageOption.__init__).parameters
    assert list(p) == ["self", "storage_type", "incremental"]
    assert p["incremental"].default is False
