"""Shared by the GRU tests: the step-by-step reference of the GRU / AUGRU
contract in whatever dtype its inputs have (fp64 = the
reference, fp32 on the CPU = the twin whose own error scales the bound of the
summed gradients), the input generator, and the error measure."""
import functools
import math

import torch

RTOL = ATOL = 1e-5      # the project's kernel bound (test_gpu_din.py)


def gru_steps(xp, wh_g, wh_c, lens, att=None):
    """out [B, T, H], h_final [B, H]: TF's GRUCell (reset gate before the
    candidate product) / VecAttGRUCell under dynamic_rnn(sequence_length)."""
    B, T, H3 = xp.shape
    H = H3 // 3
    rows, last = [], []
    for b in range(B):                       # one row at a time, one step at a time
        h = xp.new_zeros(H)
        steps = []
        for t in range(int(lens[b])):
            g = torch.sigmoid(xp[b, t, :2 * H] + h @ wh_g)
            r, u = g[:H], g[H:]
            c = torch.tanh(xp[b, t, 2 * H:] + (r * h) @ wh_c)
            if att is not None:
                u = (1.0 - att[b, t]) * u
            h = u * h + (1.0 - u) * c
            steps.append(h)
        rows.append(torch.stack(steps + [xp.new_zeros(H)] * (T - len(steps))))
        last.append(h)
    return torch.stack(rows), torch.stack(last)


def gru_steps_batched(xp, wh_g, wh_c, lens, att=None):
    """The same contract over the whole batch per step (fast enough for the
    larger shapes); checked against gru_steps in test_gru_abi.py."""
    B, T, H3 = xp.shape
    H = H3 // 3
    h = xp.new_zeros(B, H)
    outs = []
    lens = lens.reshape(B, 1)
    for t in range(T):
        g = torch.sigmoid(xp[:, t, :2 * H] + h @ wh_g)
        r, u = g[:, :H], g[:, H:]
        c = torch.tanh(xp[:, t, 2 * H:] + (r * h) @ wh_c)
        if att is not None:
            u = (1.0 - att[:, t:t + 1]) * u
        nh = u * h + (1.0 - u) * c
        live = t < lens
        outs.append(torch.where(live, nh, torch.zeros_like(nh)))
        h = torch.where(live, nh, h)
    return torch.stack(outs, 1), h


def case(B, T, I, H, seed, scale=1.0):
    """x [B, T, I] randn * scale, seq_len[0] = T, seq_len[1] = 0, the rest
    U[0, T]; Glorot-uniform kernels [I + H, .], gates bias 1, a small
    candidate bias; att a softmax row; grad_out, grad_h_final randn.  fp64."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, I, generator=g, dtype=torch.float64) * scale
    lens = torch.randint(0, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[1] = 0

    def glorot(a, b):
        lim = math.sqrt(6.0 / (a + b))
        return (torch.rand(a, b, generator=g, dtype=torch.float64) * 2 - 1) * lim
    Wg, Wc = glorot(I + H, 2 * H), glorot(I + H, H)
    bg = torch.ones(2 * H, dtype=torch.float64)
    bc = torch.randn(H, generator=g, dtype=torch.float64) * 0.1
    att = torch.softmax(torch.randn(B, T, generator=g, dtype=torch.float64) * 3, -1)
    go = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    gh = torch.randn(B, H, generator=g, dtype=torch.float64)
    return dict(x=x, lens=lens, Wg=Wg, bg=bg, Wc=Wc, bc=bc, att=att, go=go, gh=gh, I=I, H=H)


NAMES = ("out", "hT", "dxp", "dx", "dWg", "dbg", "dWc", "dbc", "datt")
SUMMED = ("dWg", "dbg", "dWc", "dbc")      # sums over the B * T positions


def run(cs, fn, dtype, device, use_att):
    """The layer as DIEN builds it (xp = x W_x + b by torch, the recurrence by
    fn) and the loss sum(out * go) + sum(h_final * gh): outputs and every
    gradient, as fp64 CPU tensors.  The fp32 runs start from the same
    fp32-rounded leaves as the fp64 one."""
    I, H = cs["I"], cs["H"]
    leaf = lambda k: cs[k].float().to(dtype).to(device).requires_grad_(True)  # noqa: E731
    x, Wg, bg, Wc, bc, att = (leaf(k) for k in ("x", "Wg", "bg", "Wc", "bc", "att"))
    lens = cs["lens"].to(device)
    xp = x @ torch.cat([Wg[:I], Wc[:I]], 1) + torch.cat([bg, bc])
    xp.retain_grad()
    out, h = fn(xp, Wg[I:], Wc[I:], lens, att if use_att else None)
    go, gh = cs["go"].float().to(dtype).to(device), cs["gh"].float().to(dtype).to(device)
    ((out * go).sum() + (h * gh).sum()).backward()
    res = [out, h, xp.grad, x.grad, Wg.grad, bg.grad, Wc.grad, bc.grad,
           att.grad if use_att else None]
    return {n: (None if v is None else v.detach().double().cpu()) for n, v in zip(NAMES, res)}


def ratio(got, want):
    """max |got - want| / (ATOL + RTOL |want|): <= 1 is within the bound."""
    if want.numel() == 0:
        return 0.0
    return float(((got - want).abs() / (ATOL + RTOL * want.abs())).max())


@functools.lru_cache(maxsize=None)
def reference(B, T, H, use_att, I=None):
    """(case, fp64 reference, fp32 CPU twin) of one shape, computed once."""
    cs = case(B, T, I or H, H, B + T + H)
    ref = run(cs, gru_steps_batched, torch.float64, "cpu", use_att)
    twin = run(cs, gru_steps_batched, torch.float32, "cpu", use_att)
    return cs, ref, twin
