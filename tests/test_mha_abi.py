"""CPU-side checks of the multi-head attention surface:
entries and header, refusals before any launch (host pointers a refused call
never dereferences), the CPU composition against the fp64 loop reference, and
one BST training step over dense tables."""
import ctypes as C
import os
import re

import pytest
import torch

import mha_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

P, I32, I64, SZ, F32 = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_float
ENTRIES = {
    "dr_mha_seq_saved_size": (SZ, [I64, I64, I64]),
    "dr_mha_seq_forward": (I32, [P, P, P, I64, P, I64, I64, I64, I64, F32, P, P, P]),
    "dr_mha_seq_backward": (I32, [P] * 3 + [I64] + [P] * 4 + [I64] * 4 + [F32] + [P] * 3 + [I64, P]),
}


@pytest.fixture(scope="module")
def lib():
    import deeprec_amd._lib as L
    lib = C.CDLL(LIB)
    for name in tuple(ENTRIES) + ("dr_last_error", "dr_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def test_entries_resolve_with_the_mirrored_signatures(lib):
    import deeprec_amd as dr
    import deeprec_amd._lib as L
    for name, sig in ENTRIES.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == sig, name
    assert lib.dr_abi_version() == 2
    assert lib.dr_mha_seq_saved_size(5, 7, 3) == 420
    assert "multihead_attention" in dr.__all__
    text = open(os.path.join(ROOT, "include", "deeprec_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"^(size_t|int) %s\(" % name, text, re.M), name


# argument positions: (head_dim, heads, T, B, row strides, pointers, 16-byte aligned, good call)
FWD = (8, 7, 6, 5, (3,), (0, 1, 2, 4, 10, 11), (0, 1, 2, 10),
       lambda a: [a, a, a, 192, a, 8, 5, 4, 16, 0.25, a, a, None])
BWD = (11, 10, 9, 8, (3, 16), (0, 1, 2, 4, 5, 6, 7, 13, 14, 15), (0, 1, 2, 5, 7, 13, 14, 15),
       lambda a: [a, a, a, 192, a, a, a, a, 8, 5, 4, 16, 0.25, a, a, a, 192, None])


@pytest.mark.parametrize("entry,pos", [("dr_mha_seq_forward", FWD), ("dr_mha_seq_backward", BWD)])
def test_bad_arguments_are_refused_before_any_launch(lib, entry, pos):
    hd, heads, T, B, lds, ptrs, aligned, good = pos
    buf = (C.c_float * 64)()
    a = C.addressof(buf)            # host memory: never dereferenced by a refused call
    a += 16 - a % 16
    fn, good = getattr(lib, entry), good(a)
    bad = [(hd, v) for v in (0, 4, 12, 24, 64)] + [(heads, v) for v in (0, -1)]
    bad += [(T, v) for v in (0, -1, 129)] + [(B, -1)]
    bad += [(ld, v) for ld in lds for v in (60, 66)]         # below E = 64; not a multiple of 4
    bad += [(k, None) for k in ptrs] + [(k, a + 4) for k in aligned]
    for k, val in bad:
        args = list(good)
        args[k] = val
        assert fn(*args) == INVALID_ARGUMENT, (k, val)
        assert b"mha" in lib.dr_last_error(), (k, val)
    args = list(good)
    args[B] = 0                                              # nothing to launch
    assert fn(*args) == 0


@pytest.mark.parametrize("B,T,heads,hd", [(5, 9, 2, 8), (3, 1, 4, 4), (4, 20, 3, 6)])
def test_multihead_attention_cpu_matches_the_fp64_loop_reference(B, T, heads, hd):
    from deeprec_amd import ops
    cs, want = mha_ref.case(B, T, heads, hd), mha_ref.reference(B, T, heads, hd)
    got = mha_ref.run(cs, ops.multihead_attention, torch.float32, "cpu")
    pad = torch.arange(T)[None, :] >= cs["lens"][:, None]
    for name in mha_ref.NAMES:
        assert mha_ref.ratio(got[name], want[name]) <= 1.0, name
        assert torch.equal(got[name][pad], torch.zeros_like(got[name][pad])), name


def test_bst_train_step_on_the_cpu():
    import deeprec_amd as dr
    from deeprec_amd import modelzoo as mz
    torch.manual_seed(3)
    D, B, T, R = 6, 7, 5, [11, 13, 5]
    tables = [dr.DenseTable(torch.randn(r, D) * 0.1) for r in R]
    model = mz.BST(*tables, max_len=T, num_units=16, num_heads=2)
    lens = torch.randint(1, T + 1, (B,))
    mask = (torch.arange(T)[None, :] < lens[:, None]).float()
    rnd = lambda r, *shape: torch.randint(1, r, shape)  # noqa: E731
    batch = (rnd(R[0], B), rnd(R[1], B), rnd(R[2], B), rnd(R[1], B, T) * mask.long(),
             rnd(R[2], B, T) * mask.long(), mask)
    lab, before, seen = (torch.rand(B) > 0.5).long(), [t.weight.clone() for t in tables], []

    class Sgd(object):
        def apply_gradients(self, tabs, global_step=None):
            for t in tabs:
                seen.append([sl.indices.clone() for sl in t.pending_grads])
                for sl in t.pending_grads:
                    t.weight.index_add_(0, sl.indices, sl.values, alpha=-0.1)
                t.pending_grads = []

    loss = mz.bst_train_step(model, batch + (torch.stack([lab, 1 - lab], 1).float(),),
                             torch.optim.SGD(model.parameters(), lr=0.1), Sgd())
    assert torch.isfinite(loss) and float(loss.detach()) > 0
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert float(p.grad.abs().max()) > 0, name
    uids, mids, cats, mid_his, cat_his, _ = batch
    want_ids = [uids, torch.cat([mids, mid_his.reshape(-1)]), torch.cat([cats, cat_his.reshape(-1)])]
    assert len(seen) == 3
    for t, (got, ids) in enumerate(zip(seen, want_ids)):
        assert len(got) == 1 and torch.equal(got[0], ids), t       # one slice: target | history
        assert not torch.equal(tables[t].weight, before[t]), t
