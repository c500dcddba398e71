"""CPU-side checks of the gate-mix surface: entries and
header, refusals before any launch (host pointers a refused call never
dereferences), the CPU composition against fp64, and one multi-task training
step of MMoE and PLE over dense tables."""
import ctypes as C
import os
import re

import pytest
import torch

import gate_mix_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
INVALID_ARGUMENT = 3

P, I32, I64, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
ENTRIES = {
    "dr_gate_mix_saved_size": (SZ, [I64, I64, I64]),
    "dr_gate_mix_forward": (I32, [P, I64, P, I64, P] + [I64] * 4 + [P, P, P]),
    "dr_gate_mix_backward": (I32, [P, I64, P, P, I64, P] + [I64] * 4 + [P, P, P]),
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
    assert lib.dr_gate_mix_saved_size(5, 3, 7) == 420
    assert "gate_mix" in dr.__all__
    text = open(os.path.join(ROOT, "include", "deeprec_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"^(size_t|int) %s\(" % name, text, re.M), name


# argument positions: (select, B, K, E, H, {stride: least}, data pointers, good call); the good
# call is K = 3, E = 5, H = 8: strides 16 >= K E, 40 = E H, 24 = K H
FWD = (4, 5, 6, 7, 8, {1: 15, 3: 40}, (0, 2, 9, 10),
       lambda a, s: [a, 16, a, 40, s, 4, 3, 5, 8, a, a, None])
BWD = (5, 6, 7, 8, 9, {1: 40, 4: 24}, (0, 2, 3, 10, 11),
       lambda a, s: [a, 40, a, a, 24, s, 4, 3, 5, 8, a, a, None])


@pytest.mark.parametrize("entry,pos", [("dr_gate_mix_forward", FWD), ("dr_gate_mix_backward", BWD)])
def test_bad_arguments_are_refused_before_any_launch(lib, entry, pos):
    sel, B, K, E, H, lds, ptrs, good = pos
    buf = (C.c_float * 64)()
    a = C.addressof(buf)            # host memory: never dereferenced by a refused call
    a += 16 - a % 16
    words = lambda *w: C.cast((C.c_uint32 * 3)(*w), P)  # noqa: E731
    fn, good = getattr(lib, entry), good(a, words(1, 18, 31))
    bad = [(K, v) for v in (0, -1, 9)] + [(E, v) for v in (0, 17)] + [(B, -1)]
    bad += [(H, v) for v in (0, 2, 6, 516, -4)]
    bad += [(ld, v) for ld, least in lds.items() for v in (least - 3, least + 2)]
    bad += [(k, None) for k in ptrs] + [(k, a + 4) for k in ptrs]
    bad += [(sel, words(1, 0, 31)), (sel, words(1, 18, 32))]        # empty; a bit at E
    for k, val in bad:
        args = list(good)
        args[k] = val
        assert fn(*args) == INVALID_ARGUMENT, (k, val)
        assert b"gate_mix" in lib.dr_last_error(), (k, val)
    for s in (good[sel], None):                                   # nothing to launch
        args = list(good)
        args[B], args[sel] = 0, s
        assert fn(*args) == 0


@pytest.mark.parametrize("case", [(5, 2, 8, 16, False), (3, 3, 5, 6, True), (4, 1, 17, 4, False)])
def test_gate_mix_cpu_matches_fp64(case):
    from deeprec_amd import ops
    cs, want = ref.case(*case), ref.reference(*case)
    got = ref.run(cs, ops.gate_mix, torch.float32, "cpu")
    for name in got:
        assert ref.ratio(got[name], want[name]) <= 1.0, name
    with pytest.raises(Exception, match="gate_mix"):
        ops.gate_mix(cs["z"][0], cs["h"])                         # wrong rank


@pytest.mark.parametrize("name", ["MMoE", "PLE"])
def test_multitask_train_step_on_the_cpu(name):
    import deeprec_amd as dr
    from deeprec_amd import modelzoo as mz
    torch.manual_seed(5)
    D, B, R = 4, 9, [11, 13, 5]
    tables = [dr.DenseTable(torch.randn(r, D) * 0.1) for r in R]
    if name == "MMoE":
        model = mz.MMoE(tables, 3, experts=3, expert_sizes=(8, 4), tasks=2, tower_sizes=(6,))
    else:
        model = mz.PLE(tables, 3, specific=2, shared=1, levels=2, expert_sizes=(8,), tasks=2,
                       tower_sizes=(6,))
    ids = torch.stack([torch.randint(0, r, (B,)) for r in R])
    labels, before = (torch.rand(B, 2) > 0.5).float(), [t.weight.clone() for t in tables]

    class Sgd(object):
        def apply_gradients(self, tabs, global_step=None):
            for t in tabs:
                for sl in t.pending_grads:
                    t.weight.index_add_(0, sl.indices, sl.values, alpha=-0.1)
                t.pending_grads = []

    loss = mz.multitask_train_step(model, torch.randn(B, 3), ids, labels,
                                   torch.optim.SGD(model.parameters(), lr=0.1), Sgd())
    assert torch.isfinite(loss) and float(loss.detach()) > 0
    for pname, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), pname
        assert float(p.grad.abs().max()) > 0, pname
        if p.dim() == 3:                                          # every expert and gate of a group
            assert (p.grad.flatten(1).abs().amax(1) > 0).all(), pname
    for t, w in zip(tables, before):
        assert not torch.equal(t.weight, w)
