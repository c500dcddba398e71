"""CPU-side checks of the CIN surface: the entries, refusals before any
launch, the CPU composition against fp64, and an xDeepFM training step over dense tables."""
import ctypes as C

import pytest
import torch

import cin_ref as ref

INVALID_ARGUMENT = 3


def test_entries_resolve_and_refuse_shapes_outside_the_native_set():
    import deeprec_amd as dr
    import deeprec_amd._lib as L
    lib = L.lib()
    for name in ("dr_cin_forward", "dr_cin_backward", "dr_cin_workspace_size"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert "cin_layer" in dr.__all__
    # one slice per column stage at most; 32 slices of [Hn, Hk, m] + [Hn] when the batch is long
    assert lib.dr_cin_workspace_size(1, 1, 1, 1, 1) == 2 * 4
    assert lib.dr_cin_workspace_size(4100, 3, 4, 16, 16) == 32 * (16 * 12 + 16) * 4
    assert lib.dr_cin_workspace_size(2, 3, 4, 16, 65) == 0
    buf = (C.c_float * 64)()
    a = C.addressof(buf)            # host memory: never dereferenced by a refused call
    for m, Hk, Hn, D in ((3, 4, 16, 65), (3, 4, 257, 16), (65, 4, 16, 16), (3, 0, 16, 16)):
        assert lib.dr_cin_forward(a, a, a, None, 2, m, Hk, Hn, D, a, None) == INVALID_ARGUMENT
        assert b"cin" in lib.dr_last_error()
        assert lib.dr_cin_backward(a, a, a, a, 2, m, Hk, Hn, D, a, a, a, None, a, 0,
                                   None) == INVALID_ARGUMENT


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] in ref.SHAPES[:3]])
@pytest.mark.parametrize("kind", ["integer", "real"])
def test_cin_layer_cpu_matches_fp64(case, kind):
    from deeprec_amd import ops
    cs, want = ref.case(*case, kind), ref.reference(*case, kind)
    got = ref.run(cs, ops.cin_layer, torch.float32, "cpu")
    for n in ref.NAMES:
        if want[n] is not None:
            assert ref.ratio(got[n], want[n]) <= (0.0 if kind == "integer" else 1.0), n
    with pytest.raises(Exception, match="cin_layer"):
        ops.cin_layer(cs["x0"][0], cs["x0"], cs["w"])       # wrong rank


def test_xdeepfm_trains_on_the_cpu_and_matches_its_formula(monkeypatch):
    import deeprec_amd as dr
    from deeprec_amd import modelzoo as mz, ops
    torch.manual_seed(11)
    B, R = 9, [11, 13, 7]
    tables = [dr.DenseTable(torch.randn(r, 4) * 0.1) for r in R]
    with pytest.raises(ValueError):
        mz.XDeepFM(tables + [dr.DenseTable(torch.randn(5, 8))], 3)
    model = mz.XDeepFM(tables, 3, cin_sizes=(6, 5), dnn_sizes=(8,))
    dense, ids = torch.randn(B, 3), torch.stack([torch.randint(0, r, (B,)) for r in R])
    labels, before = (torch.rand(B) > 0.5).float(), [t.weight.clone() for t in tables]

    pred = model(dense, ids)
    monkeypatch.setattr(ops, "_CIN_NATIVE", False)          # what DR_CIN=torch sets at import
    assert torch.equal(model(dense, ids), pred)
    emb = torch.stack([t.weight[i] for t, i in zip(tables, ids)], 1)               # [B, T, dim]
    x, xk, pooled = torch.cat([emb.flatten(1), dense], 1), emb, []
    for w, b in zip(model.cin.weights, model.cin.biases):
        xk = ref.compose(emb, xk, w, b)
        pooled.append(xk.sum(-1))
    logit = model.linear(x) + model.dnn(x) + model.cin_out(torch.cat(pooled, 1))
    assert pred.shape == (B,) and torch.allclose(pred, torch.sigmoid(logit).squeeze(1), atol=1e-6)

    class Sgd(object):
        def apply_gradients(self, tabs, global_step=None):
            for t in tabs:
                for sl in t.pending_grads:
                    t.weight.index_add_(0, sl.indices, sl.values, alpha=-0.05)
                t.pending_grads = []

    opt, losses = torch.optim.SGD(model.parameters(), lr=0.05), []
    for i in range(3):
        losses.append(float(mz.xdeepfm_train_step(model, dense, ids, labels, opt, Sgd(), i).detach()))
        for pname, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), pname
    assert losses[0] >= losses[1] >= losses[2], losses
    for t, w in zip(tables, before):
        assert not torch.equal(t.weight, w)
