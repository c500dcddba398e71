"""CPU-side checks of the adaptive-embedding surface: the header declares the
three entries (and the workspace size); they resolve through ctypes with the
signatures of the Python mirror; null or inconsistent arguments, a row width
outside the shapes and a short workspace are DR_INVALID_ARGUMENT with a
message before anything is launched (no GPU is touched: this runs without
one); dr_abi_version() stays 2; the Python surface refuses what the contract
refuses, with a reason."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

P, I32, I64, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
ENTRIES = {
    "dr_adaptive_split_workspace_size": (SZ, [I64]),
    "dr_adaptive_split": (I32, [P, P, I64, P, P, I32, P, I64, P, I32, P, P, P, P, P, P, P, P, P,
                                SZ, P]),
    "dr_adaptive_merge": (I32, [P, P, P, P, I64, P, P, P, P]),
    "dr_adaptive_grad": (I32, [P, I32, P, P, P, I64, P, P, P, P, P]),
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


def test_header_declares_the_entries_and_the_helper_the_bucket_rule():
    with open(os.path.join(ROOT, "include", "deeprec_amd.h")) as f:
        text = f.read()
    assert re.search(r"^size_t dr_adaptive_split_workspace_size\(int64_t nnz\);", text, re.M)
    assert re.search(r"^int dr_adaptive_split\(const int64_t\* uniq, const int32_t\* idx, "
                     r"int64_t nnz,", text, re.M)
    assert re.search(r"^int dr_adaptive_merge\(const int32_t\* mask_u, const int64_t\* hrow, ",
                     text, re.M)
    assert re.search(r"^int dr_adaptive_grad\(const float\* gu, int dim, ", text, re.M)
    with open(os.path.join(ROOT, "deeprec-1_amd", "csrc", "dr_adaptive.h")) as f:
        helper = f.read()
    assert "dr_adaptive_bucket(" in helper and "dr_adaptive_row_valid(" in helper


def _refused(lib, rc, what=None):
    assert rc == INVALID_ARGUMENT, what
    assert b"adaptive" in lib.dr_last_error(), what


# positions of dr_adaptive_split's arguments
(UNIQ, IDX, NNZ, NUM_U, MASK, MASK_BYTES, HASH, BUCKET, TABLE, DIM, COUNTS, MASK_U, HROW, EV_KEYS,
 EV_SRC, EV_COUNTS, NUM_EV, DEFAULTS, WS, WS_BYTES, STREAM) = range(21)


def _split_args(lib, buf, nnz=8):
    a = C.addressof(buf)      # host memory, 16-byte aligned: never dereferenced by a refused call
    a -= a % 16
    a += 16
    need = lib.dr_adaptive_split_workspace_size(nnz)
    return [a, a, nnz, a, a, 4, None, 5, a, 4, None, a, a, a, a, None, a, a, a, need, None]


def test_split_refuses_bad_arguments_before_any_launch(lib):
    buf = (C.c_float * 64)()
    good = _split_args(lib, buf)
    for k in (UNIQ, IDX, NUM_U, MASK, TABLE, MASK_U, HROW, EV_KEYS, EV_SRC, NUM_EV, DEFAULTS, WS):
        args = list(good)
        args[k] = None
        _refused(lib, lib.dr_adaptive_split(*args), k)
    for k, v in ((NNZ, -1), (NNZ, (1 << 31) - 1), (MASK_BYTES, 2), (MASK_BYTES, 0), (BUCKET, 0),
                 (BUCKET, -5), (DIM, 0), (DIM, -4), (DIM, 1028), (DIM, 258),
                 (COUNTS, good[UNIQ]), (EV_COUNTS, good[UNIQ]),     # one without the other
                 (WS_BYTES, good[WS_BYTES] - 1), (WS_BYTES, 0)):
        args = list(good)
        args[k] = v
        if k == NNZ and v > 0:
            args[WS_BYTES] = lib.dr_adaptive_split_workspace_size(v)
        _refused(lib, lib.dr_adaptive_split(*args), (k, v))
    # a width that is a multiple of 4 above 256 needs 16-byte aligned row blocks
    for k in (TABLE, DEFAULTS):
        args = list(good)
        args[DIM] = 260
        args[k] = good[k] + 4
        _refused(lib, lib.dr_adaptive_split(*args), ("alignment", k))
    # the workspace grows with nnz, and a sufficient one is asked for any nnz
    assert lib.dr_adaptive_split_workspace_size(1 << 20) > lib.dr_adaptive_split_workspace_size(8)
    assert lib.dr_adaptive_split_workspace_size(0) > 0


def test_merge_and_grad_refuse_bad_arguments(lib):
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += 16 - a % 16
    b = a + 64
    good = [a, a, a, a, 8, a, a, a, None]
    for k in range(8):
        if k == 4:
            continue
        args = list(good)
        args[k] = None
        _refused(lib, lib.dr_adaptive_merge(*args), k)
    for n in (-1, (1 << 31) - 1):
        args = list(good)
        args[4] = n
        _refused(lib, lib.dr_adaptive_merge(*args), n)
    assert lib.dr_adaptive_merge(a, a, a, a, 0, a, a, a, None) == 0     # nothing to launch
    good = [a, 4, a, a, a, 8, a, a, b, a, None]
    for k in (0, 2, 3, 4, 6, 7, 8, 9):
        args = list(good)
        args[k] = None
        _refused(lib, lib.dr_adaptive_grad(*args), k)
    for k, v in ((1, 0), (1, -4), (1, 1028), (1, 258), (5, -1), (5, (1 << 31) - 1),
                 (8, a)):                                 # ev_val must not be gu itself
        args = list(good)
        args[k] = v
        _refused(lib, lib.dr_adaptive_grad(*args), (k, v))
    args = list(good)
    args[1], args[8] = 260, b + 4                         # wide rows: 16-byte alignment
    _refused(lib, lib.dr_adaptive_grad(*args), "alignment")
    args = list(good)
    args[5] = 0
    assert lib.dr_adaptive_grad(*args) == 0


# ---------------------------------------------------------------------------
# the Python surface (host tensors and a stand-in EV: nothing reaches a device)
# ---------------------------------------------------------------------------
def _fake_ev(**kw):
    d = dict(value_dtype=torch.float32, tiered=False, dim=4, device=torch.device("cpu"),
             name="fake/ev", filter_freq=0, get_shape=lambda: (None, 4), pending_grads=[])
    d.update(kw)
    return SimpleNamespace(**d)


@pytest.fixture()
def var():
    import deeprec_amd as dr
    return dr.AdaptiveEmbeddingVariable("fake", dr.DenseTable(torch.zeros(5, 4)), _fake_ev())


def _sp(dr):
    return dr.SparseTensor(torch.tensor([[0, 0], [1, 0]]), torch.tensor([3, 4]), (2, 1))


def test_variable_members_dim_and_shape(var):
    import deeprec_amd as dr
    assert var.val_list == [var.hash_table, var.ev] and var.dim == 4 and var.bucket_size == 5
    assert var.get_shape() == (None, 4) and isinstance(var.hash_table, dr.DenseTable)
    assert {"AdaptiveEmbeddingVariable", "get_adaptive_embedding_variable",
            "adaptive_embedding_lookup_sparse"} <= set(dr.__all__)


def test_apply_gradients_takes_the_variable_as_its_two_members(var):
    from deeprec_amd.training import _expand_multihash
    other = object()
    assert _expand_multihash([var, other, var.ev]) == [var.hash_table, var.ev, other]


REFUSALS = {
    "max_norm": lambda dr, v, m: dr.embedding_lookup_sparse(v, _sp(dr), adaptive_mask_tensor=m,
                                                            max_norm=1.0),
    "tile": lambda dr, v, m: dr.embedding_lookup_sparse(v, _sp(dr), adaptive_mask_tensor=m,
                                                        combiner="tile"),
    "embedding_stack": lambda dr, v, m: dr.embedding_ops.embedding_stack(
        torch.zeros(2, 4), [v], [_sp(dr)]),
    "fused_embedding_lookup_sparse": lambda dr, v, m: dr.fused_embedding_lookup_sparse(v, _sp(dr)),
    "shards": lambda dr, v, m: dr.kv_variable_ops.refuse_tiered_evs([v], "ShardedLookup"),
    "partitions": lambda dr, v, m: dr.embedding_lookup_sparse([v, v], _sp(dr),
                                                              adaptive_mask_tensor=m),
    "float32": lambda dr, v, m: dr.AdaptiveEmbeddingVariable(
        "b", v.hash_table, _fake_ev(value_dtype=torch.bfloat16)),
    "HBM_DRAM": lambda dr, v, m: dr.AdaptiveEmbeddingVariable("b", v.hash_table,
                                                              _fake_ev(tiered=True)),
    "1 entries for 2 ids": lambda dr, v, m: dr.embedding_lookup_sparse(
        v, _sp(dr), adaptive_mask_tensor=torch.tensor([1])),
    "hash_ev_ids of 3 entries": lambda dr, v, m: dr.embedding_lookup_sparse(
        v, _sp(dr), adaptive_mask_tensor=m, hash_ev_ids=torch.tensor([1, 2, 3])),
    "without adaptive_mask_tensor": lambda dr, v, m: dr.embedding_lookup_sparse(v, _sp(dr)),
}


@pytest.mark.parametrize("word", sorted(REFUSALS))
def test_refusals_say_why(var, word):
    import deeprec_amd as dr
    with pytest.raises(dr.InvalidArgumentError, match=word):
        REFUSALS[word](dr, var, torch.tensor([1, 0]))


def test_every_public_lookup_refuses_the_same_way(var):
    import deeprec_amd as dr
    m = torch.tensor([1, 0])
    sp = _sp(dr)
    for call in (lambda: dr.safe_embedding_lookup_sparse(var, sp),
                 lambda: dr.safe_embedding_lookup_sparse(var, sp, adaptive_mask_tensor=m[:1]),
                 lambda: dr.safe_embedding_lookup_sparse(var, sp, adaptive_mask_tensor=m,
                                                         max_norm=2.0),
                 lambda: dr.embedding_lookup(var, torch.tensor([1, 2])),
                 lambda: dr.embedding_lookup(var, torch.tensor([1, 2]), adaptive_mask_tensor=m,
                                             max_norm=1.0),
                 lambda: dr.embedding_lookup([var, var], torch.tensor([1, 2]),
                                             adaptive_mask_tensor=m),
                 lambda: dr.embedding_lookup_sparse_multi([var], [sp]),
                 lambda: dr.embedding_lookup_sparse_multi([var], [sp], adaptive_masks=[m[:1]]),
                 lambda: dr.embedding_lookup_sparse_multi([var.hash_table], [sp],
                                                          adaptive_masks=[m]),
                 lambda: dr.adaptive_embedding_lookup_sparse(var, var, sp, None, None,
                                                             adaptive_mask_tensor=None),
                 lambda: dr.adaptive_embedding_lookup_sparse(var.hash_table, var.ev, sp, None,
                                                             None, bucket_size=7,
                                                             adaptive_mask_tensor=m),
                 lambda: dr.adaptive_embedding_lookup_sparse([var, var], var, sp, None, None,
                                                             adaptive_mask_tensor=m),
                 lambda: dr.embedding_lookup_sparse(var, sp,
                                                    adaptive_mask_tensor=torch.tensor([1.0, 0.0]))):
        with pytest.raises(dr.InvalidArgumentError):
            call()
