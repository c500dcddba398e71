"""CPU-side checks of the bilinear-interaction surface: the entries,
refusals before any launch, the CPU composition against fp64, and a FiBiNET training step over
dense tables."""
import ctypes as C

import pytest
import torch

import bilinear_ref as ref

INVALID_ARGUMENT = 3


def test_entries_resolve_and_refuse_shapes_outside_the_native_set():
    import deeprec_amd as dr
    import deeprec_amd._lib as L
    lib = L.lib()
    for name in ("dr_bilinear_forward", "dr_bilinear_backward", "dr_bilinear_workspace_size"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert "bilinear_interaction" in dr.__all__
    assert lib.dr_bilinear_workspace_size(0, 1, 2, 1) == 4              # one slice, one matrix
    assert 0 < lib.dr_bilinear_workspace_size(2, 4100, 64, 64) <= 64 << 20
    buf = (C.c_float * 64)()
    a = C.addressof(buf)            # host memory: never dereferenced by a refused call
    for kind, m, D in ((2, 1, 16), (2, 65, 16), (1, 4, 0), (0, 4, 65), (3, 4, 16)):
        assert lib.dr_bilinear_workspace_size(kind, 2, m, D) == 0
        assert lib.dr_bilinear_forward(a, None, a, kind, 2, m, D, a, None) == INVALID_ARGUMENT
        assert b"bilinear" in lib.dr_last_error()
        assert lib.dr_bilinear_backward(a, a, a, a, kind, 2, m, D, a, a, a, a, 0,
                                        None) == INVALID_ARGUMENT


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] in ref.SHAPES[:3]])
@pytest.mark.parametrize("values", ["integer", "real"])
def test_bilinear_interaction_cpu_matches_fp64(case, values):
    from deeprec_amd import ops
    cs, want = ref.case(*case, values), ref.reference(*case, values)
    got = ref.run(cs, case[1], ops.bilinear_interaction, torch.float32, "cpu")
    for n in ref.NAMES:
        if want[n] is not None:
            assert ref.ratio(got[n], want[n]) <= (0.0 if values == "integer" else 1.0), n
    with pytest.raises(Exception, match="bilinear_interaction"):
        ops.bilinear_interaction(cs["x"][0], cs["w"], case[1])          # wrong rank
    with pytest.raises(Exception, match="bilinear_interaction"):
        ops.bilinear_interaction(cs["x"], cs["w"][:, :, :-1], case[1])  # wrong weight shape


@pytest.mark.parametrize("kind", ref.KINDS)
def test_fibinet_trains_on_the_cpu_and_matches_its_formula(kind):
    import deeprec_amd as dr
    from deeprec_amd import modelzoo as mz
    torch.manual_seed(13)
    B, R = 9, [11, 13, 7]
    tables = [dr.DenseTable(torch.randn(r, 4) * 0.1) for r in R]
    with pytest.raises(ValueError):
        mz.FiBiNET(tables + [dr.DenseTable(torch.randn(5, 8))], 3)
    model = mz.FiBiNET(tables, 3, kind=kind, reduction=2, dnn_sizes=(8, 6))
    dense, ids = torch.randn(B, 3), torch.stack([torch.randint(0, r, (B,)) for r in R])
    labels, before = (torch.rand(B) > 0.5).float(), [t.weight.clone() for t in tables]

    pred = model(dense, ids)
    e = torch.stack([t.weight[i] for t, i in zip(tables, ids)], 1)                 # [B, T, dim]
    a = torch.relu(model.senet.excite(torch.relu(model.senet.squeeze(e.mean(-1)))))
    p, q = ref.compose(e, model.w_p, kind), ref.compose(e, model.w_q, kind, a)
    logit = (model.linear(torch.cat([e.flatten(1), dense], 1))
             + model.dnn(torch.cat([p.flatten(1), q.flatten(1), dense], 1)))
    assert pred.shape == (B,) and torch.allclose(pred, torch.sigmoid(logit).squeeze(1), atol=1e-6)

    class Sgd(object):
        def apply_gradients(self, tabs, global_step=None):
            for t in tabs:
                for sl in t.pending_grads:
                    t.weight.index_add_(0, sl.indices, sl.values, alpha=-0.05)
                t.pending_grads = []

    opt, losses = torch.optim.SGD(model.parameters(), lr=0.05), []
    for i in range(3):
        losses.append(float(mz.fibinet_train_step(model, dense, ids, labels, opt, Sgd(), i).detach()))
        for pname, prm in model.named_parameters():
            assert prm.grad is not None and torch.isfinite(prm.grad).all(), pname
    assert losses[0] >= losses[1] >= losses[2], losses
    for t, w in zip(tables, before):
        assert not torch.equal(t.weight, w)
