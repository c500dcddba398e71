"""CPU-side checks of the layer-norm surface: the entries, a refusal
before any launch, the CPU composition against fp64, and MaskNet training steps over dense
tables in both modes."""
import ctypes as C

import pytest
import torch

import layer_norm_ref as ref

INVALID_ARGUMENT = 3


def test_entries_resolve_and_refuse_a_width_outside_the_native_set():
    import deeprec_amd as dr
    import deeprec_amd._lib as L
    lib = L.lib()
    for name in ("dr_layer_norm_forward", "dr_layer_norm_backward", "dr_layer_norm_saved_size",
                 "dr_layer_norm_workspace_size"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.dr_abi_version() == 2 and "layer_norm" in dr.__all__
    assert lib.dr_layer_norm_saved_size(5) == 40
    assert lib.dr_layer_norm_workspace_size(600, 128) == 75 * 2 * 128 * 4      # 8-row tiles
    assert lib.dr_layer_norm_workspace_size(1 << 20, 16) == 1024 * 2 * 16 * 4  # the grid's cap
    buf = (C.c_float * 64)()
    a = C.addressof(buf)            # host memory: never dereferenced by a refused call
    a += 16 - a % 16
    for D in (6, 0, 1028):
        assert lib.dr_layer_norm_forward(a, 8, None, 0, a, a, None, 0, 2, D, 1, 1e-8, 0, a, a,
                                         None) == INVALID_ARGUMENT
        assert b"layer_norm" in lib.dr_last_error()


@pytest.mark.parametrize("shape", [(5, 64, 1), (2, 36, 3)])
@pytest.mark.parametrize("relu", [False, True])
def test_layer_norm_cpu_matches_fp64(shape, relu):
    from deeprec_amd import ops
    key = shape + (relu, 1e-3 if relu else 1e-8, shape[2] == 1)
    cs, want = ref.case(*key), ref.reference(*key)
    got = ref.run(cs, ops.layer_norm, torch.float32, "cpu")
    for name in got:
        assert ref.ratio(got[name], want[name]) <= 1.0, name
    with pytest.raises(Exception, match="layer_norm"):
        ops.layer_norm(cs["x"][0], cs["gain"], cs["bias"], 1e-8)      # wrong rank


@pytest.mark.parametrize("mode", ["serial", "parallel"])
def test_masknet_trains_on_the_cpu(mode):
    import deeprec_amd as dr
    from deeprec_amd import modelzoo as mz
    torch.manual_seed(7)
    B, R = 9, [11, 13]
    tables = [dr.DenseTable(torch.randn(r, 4) * 0.1) for r in R]
    model = mz.MaskNet(tables, 3, mode=mode, blocks=2, block_dim=8, head_sizes=(6,))
    dense, ids = torch.randn(B, 3), torch.stack([torch.randint(0, r, (B,)) for r in R])
    labels, before = (torch.rand(B) > 0.5).float(), [t.weight.clone() for t in tables]
    assert model(dense, ids).shape == (B,)

    class Sgd(object):
        def apply_gradients(self, tabs, global_step=None):
            for t in tabs:
                for sl in t.pending_grads:
                    t.weight.index_add_(0, sl.indices, sl.values, alpha=-0.05)
                t.pending_grads = []

    opt, losses = torch.optim.SGD(model.parameters(), lr=0.05), []
    for i in range(3):
        loss = mz.masknet_train_step(model, dense, ids, labels, opt, Sgd(), i)
        losses.append(float(loss.detach()))
        for pname, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), pname
    assert all(l == l and l < float("inf") for l in losses)
    assert losses[0] >= losses[1] >= losses[2], losses
    for t, w in zip(tables, before):
        assert not torch.equal(t.weight, w)
