"""One DIEN training step (modelzoo.DIEN / dien_train_step: merged item
lookup over [target | history | noclk history], GRU and AUGRU kernels, the
fused attention MLP, the auxiliary loss, DIN's FCN head) against a torch
model over dense tables, built the way test_din_train_step_matches_torch_
reference builds its twin, whose GRUs are the tests' own step loop.

Bounds: the loss, every dense gradient and the rows of the three EVs after the
SGD step at rtol 1e-5 / atol 1e-6 (test_gpu_din.py's model bounds) of the
twin's fp64 run.  Where the fp32 twin itself misses that bound against its
fp64 run -- gradients that pass through 2 x 23 recurrent steps and sum B * T
terms -- the native step may err by 4 x the fp32 twin's own error (the rule of
test_gpu_gru.py).

The loss is a mean over 96 samples, so most gradients here are smaller than
the atol of 1e-6 and that bound alone would pass a wrong one.  Every tensor is
therefore also held relative to its own largest element: max |error| / max
|reference| within the larger of 1e-5 (the same rtol, on the tensor's scale)
and 4 x the fp32 twin's error in that measure."""
import pytest
import torch

import gru_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = -4294967296.0     # float32(-2**32 + 1)
RTOL, ATOL = 1e-5, 1e-6


def _ratio(got, want):
    return float(((got.double() - want.double()).abs() / (ATOL + RTOL * want.double().abs())).max())


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def _twin(P, W, batch, target, dtype):
    """loss and the gradients of the dense parameters P and the tables W."""
    uids, mids, cats, mid_his, cat_his, mask, nmid, ncat = batch
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    W = [t.detach().to(dtype).clone().requires_grad_(True) for t in W]
    mask, target = mask.to(dtype), target.to(dtype)
    B, T = mid_his.shape
    c_bn = 1.0 / (1.0 + 1e-3) ** 0.5

    def lin(x, n):
        return x @ P[n + ".weight"].t() + P[n + ".bias"]

    def dice(x, n):
        mean = x.mean(0, keepdim=True)
        std = torch.sqrt(((x - mean) ** 2 + 1e-9).mean(0, keepdim=True))
        xp = torch.sigmoid((x - mean) / (std + 1e-9))
        return P[n + ".alpha"] * (1.0 - xp) * x + xp * x

    def gru(x, n, lens, att=None):
        Wg, Wc = P[n + ".gates_kernel"], P[n + ".candidate_kernel"]
        n_in = x.shape[2]
        xp = x @ torch.cat([Wg[:n_in], Wc[:n_in]], 1) + torch.cat(
            [P[n + ".gates_bias"], P[n + ".candidate_bias"]])
        return gru_ref.gru_steps_batched(xp, Wg[n_in:], Wc[n_in:], lens, att)

    def aux_prob(h, seq):
        x = torch.cat([h, seq], -1) * c_bn * P["aux_bn_gamma"] + P["aux_bn_beta"]
        x = torch.sigmoid(lin(x, "aux_f1"))
        x = torch.sigmoid(lin(x, "aux_f2"))
        return (torch.softmax(lin(x, "aux_f3"), -1) + 1e-8)[..., 0]

    emb = torch.nn.functional.embedding
    uid_e = emb(uids, W[0])
    item = torch.cat([emb(mids, W[1]), emb(cats, W[2])], 1)
    his = torch.cat([emb(mid_his, W[1]), emb(cat_his, W[2])], 2)
    noclk = torch.cat([emb(nmid, W[1]), emb(ncat, W[2])], 2)
    lens = mask.sum(1).long()
    rnn, _ = gru(his, "gru1", lens)
    click = aux_prob(rnn[:, :-1], his[:, 1:])
    noclick = aux_prob(rnn[:, :-1], noclk[:, 1:])
    aux = ((-torch.log(click) - torch.log(1.0 - noclick)) * mask[:, 1:]).mean()
    q = item.unsqueeze(1).expand(-1, T, -1)
    h = torch.sigmoid(lin(torch.cat([q, rnn, q - rnn, q * rnn], -1), "f1_att"))
    h = torch.sigmoid(lin(h, "f2_att"))
    scores = lin(h, "f3_att").view(B, T)
    alphas = torch.softmax(torch.where(mask == 1, scores, torch.full_like(scores, PAD)), -1)
    _, final2 = gru(rnn, "gru2", lens, alphas)
    his_sum = his.sum(1)
    inp = torch.cat([uid_e, item, his_sum, item * his_sum, final2], -1)
    bn = inp * c_bn * P["bn1_gamma"] + P["bn1_beta"]
    x = dice(lin(bn, "dnn1"), "dice_1")
    x = dice(lin(x, "dnn2"), "dice_2")
    y = torch.softmax(lin(x, "dnn3"), -1) + 1e-8
    loss = -(torch.log(y) * target).mean() + aux
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in P.items()}, [w.grad for w in W]


def _evs(dr, name, tables):
    evs = []
    for t, w in enumerate(tables):
        ev = dr.EmbeddingVariable("%s_%d" % (name, t), w.shape[1], 0.0, device=DEV)
        ev.insert(torch.arange(w.shape[0], device=DEV), w.to(DEV))
        evs.append(ev)
    return evs


def _ev_rows(ev, R):
    k, v = ev.export()[:2]
    out = torch.zeros(R, ev.dim, device=DEV)
    out[k] = v
    return out


def test_dien_train_step_matches_torch_reference():
    import deeprec_amd as dr
    from deeprec_amd import modelzoo as mz
    from deeprec_amd import ops
    torch.manual_seed(12)
    D, B, T, lr = 18, 96, 23, 0.05
    R = [40, 60, 12]                                    # uid, mid, cat vocab
    g = torch.Generator(device="cpu").manual_seed(5)
    tables = [torch.randn(r, D, generator=g) * 0.1 for r in R]
    evs = _evs(dr, "dien", tables)
    model = mz.DIEN(*evs).to(DEV)
    assert ops._GRU_NATIVE and 2 * D in ops.DIN_MLP_HIDDEN
    rnd = lambda r, *shape: torch.randint(1, r, shape, device=DEV)  # noqa: E731
    lens = torch.randint(1, T + 1, (B,), device=DEV)
    mask = (torch.arange(T, device=DEV)[None, :] < lens[:, None]).float()
    m = mask.long()                                                        # zero padded
    batch = (torch.randint(0, R[0], (B,), device=DEV), torch.randint(0, R[1], (B,), device=DEV),
             torch.randint(0, R[2], (B,), device=DEV), rnd(R[1], B, T) * m, rnd(R[2], B, T) * m,
             mask, rnd(R[1], B, T) * m, rnd(R[2], B, T) * m)
    lab = (torch.rand(B, device=DEV) > 0.5).long()
    target = torch.stack([lab, 1 - lab], 1).float()

    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    W = [t.to(DEV) for t in tables]
    loss64, gP64, gW64 = _twin(P, W, batch, target, torch.float64)
    loss32, gP32, gW32 = _twin(P, W, batch, target, torch.float32)

    dopt = torch.optim.SGD(model.parameters(), lr=lr)
    loss = mz.dien_train_step(model, batch + (target,), dopt, dr.GradientDescentOptimizer(lr))
    dr.status_check()

    rows = []    # (name, native, fp32 twin, reference)
    rows.append(("loss", loss.detach(), loss32, loss64))
    for name, prm in model.named_parameters():
        assert prm.grad is not None, name
        rows.append((name, prm.grad, gP32[name], gP64[name]))
    for t in range(3):
        rows.append(("ev%d rows" % t, _ev_rows(evs[t], R[t]), W[t] - lr * gW32[t],
                     W[t].double() - lr * gW64[t]))
    stats = [(name, _ratio(got, want), _ratio(twin, want), _rel(got, want), _rel(twin, want))
             for name, got, twin, want in rows]
    for name, e, te, r, tr in stats:
        print("dien %-24s error / bound: native %.3f, fp32 twin %.3f; error / scale: native "
              "%.2e, fp32 twin %.2e" % (name, e, te, r, tr))
    for name, e, te, r, tr in stats:
        assert e <= max(1.0, 4.0 * te), (name, e, te)
        if name == "f3_att.bias":
            # the softmax over T ignores a shift of all scores: this gradient is 0 (1e-19 in
            # the fp64 run) and a measure relative to it says nothing
            assert float(dict((n, w) for n, _, _, w in rows)[name].abs().max()) < 1e-12
            continue
        assert r <= max(1e-5, 4.0 * tr), (name, r, tr)
    for t in range(3):                       # every table moved, by about lr * its gradient
        moved = float((_ev_rows(evs[t], R[t]) - W[t]).abs().max())
        want = float(lr * gW64[t].abs().max())
        print("dien ev%d largest update %.3e (reference %.3e)" % (t, moved, want))
        assert 0.5 * want <= moved <= 2.0 * want, (t, moved, want)
