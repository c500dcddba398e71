"""CPU-side checks of the dense checkpoint entries (csrc/dense_ckpt.hip): they
resolve through ctypes with the signatures of the Python mirror, every refusal
the header lists is DR_INVALID_ARGUMENT before a device is touched (this test
runs without one), the ABI version stays 2, and the words function is right
at the word boundaries and at 2^31 rows."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

ENTRIES = ("dr_dense_bits_num_words", "dr_dense_mark_rows", "dr_dense_mark_all",
           "dr_dense_clear_marks", "dr_dense_marked_count",
           "dr_dense_export_marked_workspace_size", "dr_dense_export_marked",
           "dr_dense_upsert_rows")

# addresses that are never dereferenced on the host: every call below is
# refused while its arguments are validated
A16, A16B, ODD = 0x10000, 0x20000, 0x10004


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


def refused(lib, rc):
    assert rc == INVALID_ARGUMENT, rc
    assert lib.dr_last_error()


def test_entries_resolve_and_abi_version_stays(lib):
    import deeprec_amd._lib as L
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert lib.dr_abi_version() == 2
    assert L.DENSE_MAX_COLS == 4
    assert C.sizeof(L.DrDenseMarkDesc) == 40


@pytest.mark.parametrize("rows,want", [(1, 1), (31, 1), (32, 1), (33, 2), (1 << 31, 1 << 26),
                                       (0, 0), (-5, 0), (64, 2), (65, 3)])
def test_words(lib, rows, want):
    assert lib.dr_dense_bits_num_words(rows) == want


def _desc(L, bits=A16, rows=10, idx=A16B, n=4, n_dev=None):
    d = (L.DrDenseMarkDesc * 1)()
    d[0].bits, d[0].rows, d[0].idx, d[0].n, d[0].n_dev = bits, rows, idx, n, n_dev
    return d


def test_mark_refusals(lib):
    import deeprec_amd._lib as L
    refused(lib, lib.dr_dense_mark_rows(None, 1, None))
    refused(lib, lib.dr_dense_mark_rows(_desc(L), -1, None))
    refused(lib, lib.dr_dense_mark_rows(_desc(L, rows=0), 1, None))
    refused(lib, lib.dr_dense_mark_rows(_desc(L, n=-1), 1, None))
    refused(lib, lib.dr_dense_mark_rows(_desc(L, n=1 << 31), 1, None))
    refused(lib, lib.dr_dense_mark_rows(_desc(L, idx=None), 1, None))
    # nothing to do is no refusal and no launch: no tables, a skipped
    # descriptor (bits NULL, whatever else it holds), an empty index list
    assert lib.dr_dense_mark_rows(None, 0, None) == 0
    assert lib.dr_dense_mark_rows(_desc(L, bits=None, rows=-3, idx=None, n=-1), 1, None) == 0
    assert lib.dr_dense_mark_rows(_desc(L, idx=None, n=0), 1, None) == 0


def test_fill_and_count_refusals(lib):
    for fn in (lib.dr_dense_mark_all, lib.dr_dense_clear_marks):
        refused(lib, fn(None, 10, None))
        refused(lib, fn(A16, 0, None))
        refused(lib, fn(A16, -1, None))
    refused(lib, lib.dr_dense_marked_count(None, 10, A16B, None))
    refused(lib, lib.dr_dense_marked_count(A16, 10, None, None))
    refused(lib, lib.dr_dense_marked_count(A16, 0, A16B, None))


def _export(lib, bits=A16, rows=100, dim=8, cols=(A16,), ncols=None, capacity=4, rows_out=A16B,
            vals=(A16B,), m_dev=A16, ws=A16, ws_bytes=None):
    P = C.c_void_p * 8
    if ws_bytes is None:
        ws_bytes = lib.dr_dense_export_marked_workspace_size(rows)
    return lib.dr_dense_export_marked(
        bits, rows, dim, None if cols is None else P(*cols), len(cols) if ncols is None else ncols,
        capacity, rows_out, None if vals is None else P(*vals), m_dev, ws, ws_bytes, None)


def test_export_refusals(lib):
    need = lib.dr_dense_export_marked_workspace_size(100)
    assert need > 0
    assert lib.dr_dense_export_marked_workspace_size(10_000_000) > \
        2 * 4 * lib.dr_dense_bits_num_words(10_000_000)
    refused(lib, _export(lib, bits=None))
    refused(lib, _export(lib, m_dev=None))
    refused(lib, _export(lib, rows=0))
    refused(lib, _export(lib, rows=1 << 31, ws_bytes=1 << 40))
    refused(lib, _export(lib, cols=(A16,) * 5, vals=(A16B,) * 5))        # more than 4 columns
    refused(lib, _export(lib, ncols=-1))
    refused(lib, _export(lib, capacity=-1))
    refused(lib, _export(lib, cols=None, ncols=1))
    refused(lib, _export(lib, vals=None))
    refused(lib, _export(lib, rows_out=None))
    refused(lib, _export(lib, cols=(A16, None), vals=(A16B, A16B)))
    refused(lib, _export(lib, cols=(A16, A16B), vals=(A16B, None)))
    refused(lib, _export(lib, cols=(A16,), vals=(A16,)))                 # onto itself
    # widths: 0, above 1024, above 256 when not a multiple of 4 or not aligned
    refused(lib, _export(lib, dim=0))
    refused(lib, _export(lib, dim=1028))
    refused(lib, _export(lib, dim=258))
    refused(lib, _export(lib, dim=260, cols=(ODD,)))
    refused(lib, _export(lib, dim=260, vals=(ODD,)))
    # workspace: missing, or one byte short
    refused(lib, _export(lib, ws=None))
    refused(lib, _export(lib, ws_bytes=need - 1))


def _upsert(lib, cols=(A16,), ncols=None, rows=100, dim=8, idx=A16B, n=4, n_dev=None,
            vals=(A16B,)):
    P = C.c_void_p * 8
    return lib.dr_dense_upsert_rows(
        None if cols is None else P(*cols), len(cols) if ncols is None else ncols, rows, dim, idx,
        n, n_dev, None if vals is None else P(*vals), None)


def test_upsert_refusals(lib):
    refused(lib, _upsert(lib, cols=None, ncols=1))
    refused(lib, _upsert(lib, vals=None))
    refused(lib, _upsert(lib, ncols=0))
    refused(lib, _upsert(lib, cols=(A16,) * 5, vals=(A16B,) * 5))
    refused(lib, _upsert(lib, rows=0))
    refused(lib, _upsert(lib, n=-1))
    refused(lib, _upsert(lib, n=1 << 31))
    refused(lib, _upsert(lib, idx=None))
    refused(lib, _upsert(lib, cols=(None,)))
    refused(lib, _upsert(lib, vals=(None,)))
    refused(lib, _upsert(lib, cols=(A16,), vals=(A16,)))
    refused(lib, _upsert(lib, cols=(A16, A16), vals=(A16B, A16B + 0x1000)))   # one block twice
    refused(lib, _upsert(lib, dim=0))
    refused(lib, _upsert(lib, dim=1028))
    refused(lib, _upsert(lib, dim=258))
    refused(lib, _upsert(lib, dim=260, vals=(ODD,)))
    # an empty delta is no refusal and no launch
    assert _upsert(lib, n=0, idx=None, vals=(None,)) == 0


def test_python_surface_exists():
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    for name in ("track_updates", "tracking_updates", "mark_updated", "updated_count",
                 "export_updated", "clear_updated", "upsert"):
        assert callable(getattr(dr.DenseTable, name)), name
    for opt in (dr.GradientDescentOptimizer, dr.AdagradOptimizer, dr.AdamOptimizer,
                dr.FtrlOptimizer, dr.AdamAsyncOptimizer, dr.AdagradDecayOptimizer):
        assert callable(opt.checkpoint_variables)
    assert callable(ck.expand_variables)
