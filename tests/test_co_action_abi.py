"""CPU-side checks of the co-action surface: the entries, refusals before
any launch, the CPU composition against fp64, and a CAN training step over dense tables."""
import ctypes as C

import pytest
import torch

import co_action_ref as ref

INVALID_ARGUMENT = 3


def test_entries_resolve_and_refuse_arguments_outside_the_native_set():
    import deeprec_amd as dr
    import deeprec_amd._lib as L
    lib = L.lib()
    for name in ("dr_co_action_forward", "dr_co_action_backward"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert "co_action" in dr.__all__
    buf = (C.c_float * 64)()
    a = C.addressof(buf)            # host memory: never dereferenced by a refused call
    ok = dict(widths=(16, 8, 4), orders=3, ld_p=160, ld_h=16, T=5)
    bad = [dict(widths=(16, 6, 4)), dict(widths=(36, 8, 4)), dict(widths=(16, 8, 0)),
           dict(widths=(16,)), dict(widths=(16, 8, 4, 4, 4)), dict(orders=0), dict(orders=5),
           dict(ld_p=162), dict(ld_p=156), dict(ld_h=18), dict(ld_h=12), dict(T=0)]
    for change in bad:
        k = dict(ok, **change)
        w = (C.c_int * len(k["widths"]))(*k["widths"])
        tail = (2, k["T"], w, len(k["widths"]) - 1, k["orders"], 0, 0)
        assert lib.dr_co_action_forward(a, k["ld_p"], a, k["ld_h"], a, *tail, a,
                                        None) == INVALID_ARGUMENT, change
        assert b"co_action" in lib.dr_last_error()
        assert lib.dr_co_action_backward(a, k["ld_p"], a, k["ld_h"], a, a, *tail, a, a,
                                         None) == INVALID_ARGUMENT, change
    w = (C.c_int * 3)(16, 8, 4)     # an empty batch is served without a launch
    assert lib.dr_co_action_forward(a, 160, a, 16, a, 0, 5, w, 2, 3, 0, 0, a, None) == 0
    assert lib.dr_co_action_backward(a, 160, a, 16, a, a, 0, 5, w, 2, 3, 0, 0, a, a, None) == 0


@pytest.mark.parametrize("key", ref.CASES[:4])
def test_co_action_cpu_matches_fp64(key):
    from deeprec_amd import ops
    cs, want = ref.case(key, "real"), ref.reference(key, "real")
    got = ref.run(key, cs, ops.co_action, torch.float32, "cpu")
    for n in ref.NAMES:
        assert ref.ratio(got[n], want[n]) <= 1.0, n
    with pytest.raises(Exception, match="co_action"):
        ops.co_action(cs["param"], cs["his"][0], cs["mask"], *key[2:])     # wrong rank


def test_can_trains_on_the_cpu_and_matches_its_formula():
    import deeprec_amd as dr
    from deeprec_amd import modelzoo as mz
    torch.manual_seed(13)
    B, T, D, widths, orders = 9, 6, 8, (8, 4, 4), 2
    P = ref.param_len(widths, orders, False, False)
    table = lambda rows, dim, s: dr.DenseTable(torch.randn(rows, dim) * s)  # noqa: E731
    tables = [table(11, 4, 0.1), table(13, D, 0.5), table(7, D, 0.5), table(13, P, 0.3),
              table(7, P, 0.3)]
    with pytest.raises(ValueError):
        mz.CAN(*tables[:3], table(13, P + 4, 0.3), tables[4], widths, orders)
    with pytest.raises(ValueError):
        mz.CAN(tables[0], table(13, D + 4, 0.5), *tables[2:], widths, orders)
    model = mz.CAN(*tables, widths, orders)
    assert model.evs == tables
    mask = (torch.rand(B, T) < 0.7).float()
    uids, mids, cats = (torch.randint(0, r, (B,)) for r in (11, 13, 7))
    mid_his, cat_his = torch.randint(0, 13, (B, T)), torch.randint(0, 7, (B, T))
    lab = (torch.rand(B) > 0.5).long()
    batch = (uids, mids, cats, mid_his, cat_his, mask, torch.stack([lab, 1 - lab], 1).float())
    before = [t.weight.clone() for t in tables]

    pred = model(*batch[:-1])
    uw, mw, cw, mp, cp = before
    his = torch.cat([mw[mid_his], cw[cat_his]], -1)
    item, his_sum = torch.cat([mw[mids], cw[cats]], -1), his.sum(1)
    co = [ref.compose(p, h, mask, widths, orders, False, False)
          for p, h in ((mp[mids], his[..., :D]), (cp[cats], his[..., D:]))]
    inp = torch.cat([uw[uids], item, his_sum, item * his_sum] + co, -1)
    x = inp * (1.0 + 1e-3) ** -0.5 * model.bn1_gamma + model.bn1_beta
    x = model.dice_2(model.dnn2(model.dice_1(model.dnn1(x))))
    want = torch.softmax(model.dnn3(x), -1) + 1e-8
    assert pred.shape == (B, 2) and torch.allclose(pred, want, atol=1e-6)

    class Sgd(object):
        def apply_gradients(self, tabs, global_step=None):
            for t in tabs:
                for sl in t.pending_grads:
                    t.weight.index_add_(0, sl.indices, sl.values, alpha=-0.05)
                t.pending_grads = []

    opt, losses = torch.optim.SGD(model.parameters(), lr=0.05), []
    for i in range(3):
        losses.append(float(mz.can_train_step(model, batch, opt, Sgd(), i).detach()))
        for pname, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), pname
    assert losses[0] >= losses[1] >= losses[2], losses
    for t, w in zip(tables, before):
        assert not torch.equal(t.weight, w)
