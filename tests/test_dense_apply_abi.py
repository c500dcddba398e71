"""CPU-side checks of the grouped dense-table apply: the header declares the
descriptor and the two entries; they resolve through ctypes with the
signatures of the Python mirror; an unknown optimizer, null or inconsistent
descriptors and a short workspace are DR_INVALID_ARGUMENT with a message
before anything is launched (no GPU is touched: this runs without one).

dr_abi_version(): the entries are additions, no signature changed, so the
version stays 2 -- as every earlier additive change left it (the other
*_abi tests pin the same value)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3
MAX_GROUP = 32
SGD, ADAGRAD, ADAM, ADAM_ASYNC, RMSPROP = 0, 1, 2, 3, 4

P, I32, F32, SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t
ENTRIES = {
    "dr_dense_apply_grouped_workspace_size": (SZ, [P, I32]),
    "dr_dense_apply_grouped": (I32, [I32, P, I32, F32, F32, F32, F32, P, SZ, P]),
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


def test_header_declares_the_descriptor_and_the_entries():
    with open(os.path.join(ROOT, "include", "deeprec_amd.h")) as f:
        text = f.read()
    assert re.search(r"^size_t dr_dense_apply_grouped_workspace_size\(const dr_dense_apply_desc\* "
                     r"descs_host,\s+int num_tables\);", text, re.M)
    assert re.search(r"^int dr_dense_apply_grouped\(int optimizer, const dr_dense_apply_desc\* "
                     r"descs_host, int num_tables,\s+float lr, float beta1, float beta2, "
                     r"float epsilon, void\* ws,\s+size_t ws_bytes, void\* stream\);", text, re.M)
    body = re.search(r"typedef struct \{([^}]*)\} dr_dense_apply_desc;", text).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, re.M)
    import deeprec_amd._lib as L
    assert fields == [n for n, _ in L.DrDenseApplyDesc._fields_]
    for name, code in (("DR_OPT_SGD", 0), ("DR_OPT_ADAGRAD", 1), ("DR_OPT_ADAM_ASYNC", 3),
                       ("DR_OPT_ADAM_ASYNC_RMSPROP", 4)):
        assert re.search(r"^\s+%s = %d,?$" % (name, code), text, re.M), name


def test_element_math_is_shared_with_the_ev_kernels():
    """One definition of the element updates: the header holds them, ev.hip
    and dense_apply.hip include it and define none of their own."""
    src = os.path.join(ROOT, "deeprec-1_amd", "csrc")
    with open(os.path.join(src, "dr_opt_elem.h")) as f:
        hdr = f.read()
    assert "struct OptScalars" in hdr and "float apply_one(" in hdr
    assert "float adagrad_decay_one(" in hdr
    for name in ("ev.hip", "dense_apply.hip"):
        with open(os.path.join(src, name)) as f:
            text = f.read()
        assert '#include "dr_opt_elem.h"' in text, name
        assert "struct OptScalars" not in text and "float apply_one(" not in text, name


def _desc(L, buf, **kw):
    d = L.DrDenseApplyDesc()
    a = C.addressof(buf)
    d.table, d.rows, d.dim = a, 7, 4
    d.slot1, d.slot2, d.powers = a + 256, a + 512, a + 768
    d.grad, d.idx, d.n, d.n_dev = a + 1024, a + 2048, 8, None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, rc, word=b"dense apply"):
    assert rc == INVALID_ARGUMENT
    assert word in lib.dr_last_error()


def _call(lib, L, opt, descs, n=None, ws=None, ws_bytes=0):
    arr = (L.DrDenseApplyDesc * max(len(descs), 1))(*descs)
    return lib.dr_dense_apply_grouped(opt, arr, len(descs) if n is None else n, 0.05, 0.9, 0.999,
                                      1e-8, ws, ws_bytes, None)


def test_refusals_happen_before_any_launch(lib):
    import deeprec_amd._lib as L
    buf = (C.c_float * 1024)()       # host memory: never dereferenced by a refused call
    wsbuf = (C.c_char * (1 << 16))()
    ws = C.addressof(wsbuf)
    good = _desc(L, buf)
    other = _desc(L, buf, table=C.addressof(buf) + 128)
    need = lib.dr_dense_apply_grouped_workspace_size((L.DrDenseApplyDesc * 2)(good, other), 2)
    assert 0 < need <= len(wsbuf)
    # unknown optimizers: dense Adam and anything outside the enum
    for opt in (ADAM, 5, -1, 99):
        _refused(lib, _call(lib, L, opt, [good], ws=ws, ws_bytes=len(wsbuf)))
    _refused(lib, _call(lib, L, SGD, [good], n=-1, ws=ws, ws_bytes=len(wsbuf)))
    _refused(lib, lib.dr_dense_apply_grouped(SGD, None, 1, 0.05, 0.0, 0.0, 0.0, ws, len(wsbuf),
                                             None))
    for opt, bad in ((SGD, dict(table=None)), (SGD, dict(rows=0)), (SGD, dict(dim=0)),
                     (SGD, dict(n=-1)), (SGD, dict(grad=None)), (SGD, dict(idx=None)),
                     (ADAGRAD, dict(slot1=None)), (ADAM_ASYNC, dict(slot1=None)),
                     (ADAM_ASYNC, dict(slot2=None)), (RMSPROP, dict(slot2=None)),
                     (ADAM_ASYNC, dict(powers=None)), (SGD, dict(dim=1028)),
                     (SGD, dict(dim=258)), (SGD, dict(n=1 << 31)),
                     (SGD, dict(n=(1 << 63) - 1))):
        _refused(lib, _call(lib, L, opt, [other, _desc(L, buf, **bad)], ws=ws,
                            ws_bytes=len(wsbuf)))
    # two descriptors on one table, also when they are more than a group apart
    _refused(lib, _call(lib, L, SGD, [good, other, good], ws=ws, ws_bytes=len(wsbuf)), b"same table")
    many = [_desc(L, buf, table=C.addressof(buf) + 16 * k, n=0) for k in range(MAX_GROUP + 2)]
    _refused(lib, _call(lib, L, SGD, many + [many[0]], ws=ws, ws_bytes=len(wsbuf)), b"same table")
    # a group whose positions do not fit int32
    big = [_desc(L, buf, table=C.addressof(buf) + 16 * k, n=(1 << 30)) for k in range(2)]
    _refused(lib, _call(lib, L, SGD, big, ws=ws, ws_bytes=1 << 40), b"2^31")
    # a short or missing workspace
    _refused(lib, _call(lib, L, SGD, [good, other], ws=ws, ws_bytes=need - 1), b"workspace")
    _refused(lib, _call(lib, L, SGD, [good, other], ws=None, ws_bytes=need), b"workspace")
    # nothing to do is not an error: no tables, or tables without entries
    assert _call(lib, L, SGD, [], n=0) == 0
    assert lib.dr_dense_apply_grouped_workspace_size(None, 0) == 0
    assert _call(lib, L, ADAM_ASYNC, many) == 0      # every n == 0: no launch, no workspace
    # RMSprop does not use the powers
    assert _call(lib, L, RMSPROP, [_desc(L, buf, powers=None, n=0)]) == 0


def test_workspace_size_is_the_largest_group(lib):
    import deeprec_amd._lib as L
    buf = (C.c_float * 1024)()
    one = (L.DrDenseApplyDesc * 1)(_desc(L, buf, n=1000))
    w1 = lib.dr_dense_apply_grouped_workspace_size(one, 1)
    # 33 tables: the 33rd is a group of its own, the workspace is reused
    descs = [_desc(L, buf, table=C.addressof(buf) + 16 * k, n=10) for k in range(MAX_GROUP)]
    arr = (L.DrDenseApplyDesc * (MAX_GROUP + 1))(*(descs + [one[0]]))
    assert lib.dr_dense_apply_grouped_workspace_size(arr, MAX_GROUP + 1) == w1
    assert lib.dr_dense_apply_grouped_workspace_size(arr, MAX_GROUP) < w1
    # tables of different row shapes never share a launch group: a 4-wide and
    # a scalar table of 1000 positions each need one table's workspace
    a = C.addressof(buf)
    mixed = (L.DrDenseApplyDesc * 3)(_desc(L, buf, n=1000), _desc(L, buf, table=a + 16, dim=6, n=1000),
                                     _desc(L, buf, table=a + 32, dim=512, n=1000))
    assert lib.dr_dense_apply_grouped_workspace_size(mixed, 3) == w1
    same = (L.DrDenseApplyDesc * 2)(_desc(L, buf, n=1000), _desc(L, buf, table=a + 16, n=1000))
    assert lib.dr_dense_apply_grouped_workspace_size(same, 2) > w1


def test_the_torch_arm_is_selected_by_the_environment():
    import sys
    # one fresh interpreter (the flag is read at import): unset, torch, native
    code = ("import os, importlib\n"
            "os.environ.pop('DR_DENSE_APPLY', None)\n"
            "import deeprec_amd.training as t\n"
            "out = [t._NATIVE_DENSE]\n"
            "for v in ('torch', 'native'):\n"
            "    os.environ['DR_DENSE_APPLY'] = v\n"
            "    out.append(importlib.reload(t)._NATIVE_DENSE)\n"
            "print(out)\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [os.path.join(ROOT, "deeprec-1_amd")] + [p for p in sys.path if p]))
    out = subprocess.check_output([sys.executable, "-c", code], env=env)
    assert out.decode().strip() == "[True, False, True]"
