"""CPU-side checks of the MultiHashVariable surface: the header declares the
descriptor, the operation codes and the three entries; they resolve through
ctypes with the signatures of the Python mirror; null or inconsistent
arguments are DR_INVALID_ARGUMENT with a message before anything is launched
(no GPU is touched: this runs without one); the Python constructor validates
and reports dim / get_shape."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3
MAX_GROUP = 32

P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
ENTRIES = {
    "dr_mhv_lookup_sparse_grouped": (I32, [P, I32, I64, P]),
    "dr_mhv_gather": (I32, [P, I64, I32, P, I64, I32, I32, P, I64, P, P, P]),
    "dr_mhv_grad": (I32, [P, I64, I32, P, I64, I32, I32, P, P, I64, P, P, P, P, P, P]),
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


def test_entries_resolve_with_the_mirrored_signatures(lib):
    import deeprec_amd._lib as L
    for name, sig in ENTRIES.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == sig, name
    assert lib.dr_abi_version() == 2
    assert L.MHV_OPERATIONS == {"add": 0, "mul": 1, "concat": 2}


def test_header_declares_the_descriptor_the_codes_and_the_entries():
    with open(os.path.join(ROOT, "include", "deeprec_amd.h")) as f:
        text = f.read()
    for name, code in (("DR_MHV_ADD", 0), ("DR_MHV_MUL", 1), ("DR_MHV_CONCAT", 2)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, code), text, re.M), name
    assert re.search(r"^int dr_mhv_lookup_sparse_grouped\(const dr_mhv_desc\* descs_host, "
                     r"int num_tables, int64_t batch,\s+void\* stream\);", text, re.M)
    assert re.search(r"^int dr_mhv_gather\(const float\* q_table, int64_t q_rows, int q_dim, ",
                     text, re.M)
    assert re.search(r"^int dr_mhv_grad\(const float\* q_table, int64_t q_rows, int q_dim, ",
                     text, re.M)
    body = re.search(r"typedef struct \{([^}]*)\} dr_mhv_desc;", text).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, re.M)
    import deeprec_amd._lib as L
    assert fields == [n for n, _ in L.DrMhvDesc._fields_]
    # the helper header carries the same codes and the one index rule
    with open(os.path.join(ROOT, "deeprec-1_amd", "csrc", "dr_multihash.h")) as f:
        helper = f.read()
    for name, code in (("DR_MHV_ADD", 0), ("DR_MHV_MUL", 1), ("DR_MHV_CONCAT", 2)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, code), helper, re.M), name
    assert "dr_mhv_index(" in helper


def _desc(L, buf, **kw):
    d = L.DrMhvDesc()
    a = C.addressof(buf)
    d.q_table, d.q_rows, d.q_dim = a, 7, 4
    d.r_table, d.r_rows, d.r_dim = a, 5, 4
    d.operation, d.combiner = 0, 0
    d.ids, d.bag_off, d.weights, d.out, d.out_stride = a, a, None, a, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, rc):
    assert rc == INVALID_ARGUMENT
    assert lib.dr_last_error()


def test_lookup_refuses_bad_descriptors_before_any_launch(lib):
    import deeprec_amd._lib as L
    buf = (C.c_float * 64)()       # host memory: never dereferenced by a refused call
    good = _desc(L, buf)
    _refused(lib, lib.dr_mhv_lookup_sparse_grouped(None, 1, 8, None))
    for n in (0, -1, MAX_GROUP + 1):
        arr = (L.DrMhvDesc * (MAX_GROUP + 1))(*[good] * (MAX_GROUP + 1))
        _refused(lib, lib.dr_mhv_lookup_sparse_grouped(arr, n, 8, None))
    _refused(lib, lib.dr_mhv_lookup_sparse_grouped((L.DrMhvDesc * 1)(good), 1, -1, None))
    for bad in (dict(q_table=None), dict(r_table=None), dict(ids=None), dict(out=None),
                dict(operation=3), dict(operation=-1), dict(r_dim=6),
                dict(q_rows=0), dict(r_rows=-5), dict(q_dim=0), dict(r_dim=-4),
                dict(combiner=3), dict(out_stride=3), dict(out_stride=-4),
                dict(operation=2, out_stride=7),
                dict(bag_off=None, weights=C.addressof(buf)),
                dict(q_dim=1028, r_dim=1028, out_stride=1028),
                dict(q_dim=258, r_dim=258, out_stride=258)):
        arr = (L.DrMhvDesc * 2)(good, _desc(L, buf, **bad))
        _refused(lib, lib.dr_mhv_lookup_sparse_grouped(arr, 2, 8, None))
        assert b"multihash" in lib.dr_last_error(), bad
    # concat may have unequal dims: only its out_stride was short above
    # (a well-formed call with batch 0 has nothing to launch)
    arr = (L.DrMhvDesc * 1)(_desc(L, buf, operation=2, r_dim=6, out_stride=10))
    assert lib.dr_mhv_lookup_sparse_grouped(arr, 1, 0, None) == 0


def test_gather_and_grad_refuse_bad_arguments(lib):
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    b = a + 64
    ok = [a, 7, 4, a, 5, 4, 0]
    for bad in ([None, 7, 4, a, 5, 4, 0], [a, 7, 4, None, 5, 4, 0], [a, 0, 4, a, 5, 4, 0],
                [a, 7, 4, a, -1, 4, 0], [a, 7, 4, a, 5, 6, 0], [a, 7, 4, a, 5, 6, 1],
                [a, 7, 4, a, 5, 4, 3], [a, 7, -4, a, 5, -4, 0]):
        _refused(lib, lib.dr_mhv_gather(*bad, a, 4, None, a, None))
        _refused(lib, lib.dr_mhv_grad(*bad, a, a, 4, None, a, b, a, b, None))
    _refused(lib, lib.dr_mhv_gather(*ok, None, 4, None, a, None))
    _refused(lib, lib.dr_mhv_gather(*ok, a, 4, None, None, None))
    _refused(lib, lib.dr_mhv_gather(*ok, a, -1, None, a, None))
    assert lib.dr_mhv_gather(*ok, a, 0, None, a, None) == 0
    for k in range(7, 15):
        args = ok + [a, a, 4, None, a, b, a, b, None]
        if k == 9 or k == 10:
            continue            # n, n_dev (nullable)
        args[k] = None
        _refused(lib, lib.dr_mhv_grad(*args))
    _refused(lib, lib.dr_mhv_grad(*ok, a, a, -1, None, a, b, a, b, None))
    # one value block for both slices: add only; the index blocks never coincide
    _refused(lib, lib.dr_mhv_grad(a, 7, 4, a, 5, 4, 1, a, a, 4, None, a, b, a, a, None))
    _refused(lib, lib.dr_mhv_grad(*ok, a, a, 4, None, a, a, a, b, None))
    assert lib.dr_mhv_grad(*ok, a, a, 0, None, a, b, a, a, None) == 0


def test_construction_dim_and_shape():
    import torch
    import deeprec_amd as dr
    for op, dims, dim in (("add", [[7, 4], [5, 4]], 4), ("mul", [[7, 6], [5, 6]], 6),
                          ("concat", [[7, 8], [5, 4]], 12)):
        v = dr.get_multihash_variable("v_" + op, dims, operation=op, device="cpu")
        assert isinstance(v, dr.MultiHashVariable)
        assert v.dim == dim and v.get_shape() == (49, dim)
        assert v.name == "v_" + op and v.device == torch.device("cpu")
        assert v.val_list is v._val_list and len(v.val_list) == 2
        assert [t.name for t in v.val_list] == ["v_%s/Q" % op, "v_%s/R" % op]
        assert all(isinstance(t, dr.DenseTable) and t.weight.dtype == torch.float32
                   for t in v.val_list)
        assert [list(t.get_shape()) for t in v.val_list] == dims
        assert isinstance(v.mhvconfig, dr.MultiHashVariableConfig)
        assert (v.mhvconfig.size, v.mhvconfig.strategy, v.mhvconfig.operation) == \
            (dims, "Q-R", op)
    # initializers: a callable gets each table's shape, a tensor is taken as is
    seen = []
    v = dr.get_multihash_variable("c", [[7, 4], [5, 4]], device="cpu",
                                  initializer=lambda s: seen.append(tuple(s)) or torch.ones(s))
    assert seen == [(7, 4), (5, 4)] and v.val_list[1].weight.sum().item() == 20
    w = torch.arange(20.0).reshape(5, 4)
    v = dr.get_multihash_variable("t", [[5, 4], [5, 4]], device="cpu", initializer=w)
    assert torch.equal(v.val_list[0].weight, w) and torch.equal(v.val_list[1].weight, w)
    v = dr.get_multihash_variable("p", [[7, 4], [5, 4]], device="cpu",
                                  initializer=[torch.ones(7, 4), 2.0])
    assert v.val_list[1].weight.unique().tolist() == [2.0]


@pytest.mark.parametrize("kw,word", [
    (dict(complementary_strategy="Q-R-X"), "complementary_strategy"),
    (dict(operation="sub"), "operation"),
    (dict(dims=[[7, 4]]), "dims"),
    (dict(dims=[[7, 4], [5, 4], [3, 4]]), "dims"),
    (dict(dims=[[7, 4], [5]]), "dims"),
    (dict(dims=[[0, 4], [5, 4]]), "dims"),
    (dict(dims=[[7, 4], [5, 0]]), "dims"),
    (dict(dims=[[7, 4], [5, -4]]), "dims"),
    (dict(dims="ab"), "dims"),
    (dict(dims=[[7, 4], [5, 6]], operation="add"), "dims"),
    (dict(dims=[[7, 4], [5, 6]], operation="mul"), "dims"),
])
def test_construction_refusals_name_the_argument(kw, word):
    import deeprec_amd as dr
    args = dict(dims=[[7, 4], [5, 4]], device="cpu")
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        dr.get_multihash_variable("bad", **args)


def test_non_fp32_tables_are_refused():
    import torch
    import deeprec_amd as dr
    with pytest.raises(TypeError, match="float32"):
        dr.get_multihash_variable("h", [[5, 4], [5, 4]], device="cpu",
                                  initializer=torch.zeros(5, 4, dtype=torch.float16))
    with pytest.raises(TypeError, match="float32"):
        dr.get_multihash_variable("h", [[5, 4], [5, 4]], device="cpu",
                                  initializer=lambda s: torch.zeros(s, dtype=torch.float64))
