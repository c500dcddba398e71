"""CPU-side checks of the EV init table (dr_ev_set_init_table and its two
queries): the header declares the entries and the row limit, they resolve
through ctypes with the signatures of the Python mirror, a null EV is refused
before any device is touched, and the InitializerOption surface validates
without a GPU."""
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
    "dr_ev_set_init_table": (I32, [P, P, I64, P]),
    "dr_ev_init_table_rows": (I64, [P]),
    "dr_ev_init_table": (P, [P]),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "deeprec-1_amd")])
    import deeprec_amd._lib as L
    lib = C.CDLL(LIB)
    for name in tuple(ENTRIES) + ("dr_last_error",):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def test_entries_resolve_with_the_mirrored_signatures(lib):
    import deeprec_amd._lib as L
    for name, sig in ENTRIES.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == sig, name


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "deeprec_amd.h")) as f:
        text = f.read()
    assert re.search(r"^int dr_ev_set_init_table\(dr_ev\* ev, const void\* table_host, "
                     r"int64_t rows, void\* stream\);", text, re.M)
    assert re.search(r"^int64_t dr_ev_init_table_rows\(dr_ev\* ev\);", text, re.M)
    assert re.search(r"^const float\* dr_ev_init_table\(dr_ev\* ev\);", text, re.M)
    assert re.search(r"^#define\s+DR_MAX_INIT_TABLE_ROWS\s+\(1 << 20\)", text, re.M)


def test_null_ev_is_refused_before_any_device_call(lib):
    buf = (C.c_float * 8)()
    for rows in (0, 1, 4096, (1 << 20) + 1):
        assert lib.dr_ev_set_init_table(None, buf, rows, None) == INVALID_ARGUMENT
        assert lib.dr_last_error()
    assert lib.dr_ev_init_table_rows(None) == 1
    assert not lib.dr_ev_init_table(None)


def test_initializer_option_surface():
    import torch
    import deeprec_amd as dr
    from deeprec_amd import kv_variable_ops as kvo
    p = inspect.signature(dr.InitializerOption.__init__).parameters
    assert list(p) == ["self", "initializer", "default_value_dim", "default_value_no_permission"]
    assert (p["initializer"].default, p["default_value_dim"].default,
            p["default_value_no_permission"].default) == (None, 4096, 0.0)
    assert dr.EmbeddingVariableOption().init_option is None
    io = dr.InitializerOption(0.5, 7)
    o = dr.EmbeddingVariableOption(filter_option=dr.CounterFilter(2))
    assert o.with_init_option(io) is o and o.init_option is io and o.filter_option.filter_freq == 2
    assert dr.EmbeddingVariableOption().init_option is None        # per instance
    assert isinstance(dr.EmbeddingVariable.init_table, property)
    assert kvo.MAX_INIT_TABLE_ROWS == 1 << 20
    for bad in (0, -3, (1 << 20) + 1):
        with pytest.raises(dr.InvalidArgumentError):
            dr.InitializerOption(default_value_dim=bad)
    assert dr.InitializerOption(default_value_dim=1 << 20).default_value_dim == 1 << 20
    # the table: the option's initializer first, else the EV's; a constant is broadcast
    io = dr.InitializerOption(lambda s: torch.arange(s[0] * s[1]).reshape(s), 3, 0.25)
    t = kvo._init_table_host(io, 9.0, 4)
    assert t.dtype == torch.float32 and t.tolist() == torch.arange(12.0).reshape(3, 4).tolist()
    t = kvo._init_table_host(dr.InitializerOption(None, 2), lambda s: torch.full(s, 7.0), 4,
                             torch.float64)
    assert t.dtype == torch.float64 and t.tolist() == [[7.0] * 4] * 2
    assert kvo._init_table_host(dr.InitializerOption(1.5, 2), None, 3).tolist() == [[1.5] * 3] * 2
    assert kvo._init_table_host(dr.InitializerOption(None, 2), None, 3).tolist() == [[0.0] * 3] * 2
    with pytest.raises(dr.InvalidArgumentError):
        kvo._init_table_host(dr.InitializerOption(lambda s: torch.zeros(s[0], s[1] + 1), 2), None, 3)
    with pytest.raises(dr.InvalidArgumentError):
        kvo._init_table_host(dr.InitializerOption(lambda s: torch.zeros(s[1]), 2), None, 3)
    io = dr.InitializerOption(None, 2)
    io.default_value_dim = 0
    with pytest.raises(dr.InvalidArgumentError):
        kvo._init_table_host(io, None, 3)


def test_every_initializer_gate_is_the_one_predicate():
    """embedding_ops gates its grouped / fused / recorded-rows routes on
    'draws defaults per call', not on callable(initializer)."""
    from deeprec_amd import embedding_ops as eo
    src = inspect.getsource(eo)
    assert "callable(" not in src
    for fn in (eo._prepare_all, eo._groupable, eo._rows_eligible, eo._fused_onehot_ok):
        assert "_draws_defaults(" in inspect.getsource(fn), fn.__name__
