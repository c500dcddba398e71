"""Seeded cases and the fp64 reference of the co-action tests."""
import functools

import torch

NAMES = ("out", "dhis", "dparam")
TOL = 1e-5          # rtol = atol: the project's kernel bound

# (B, T, widths, orders, bias, order_indep): every minimum; the reference configuration, one
# partial tile; a full tile plus one position, bias, B not a multiple of the waves of a block;
# widths that are no multiples of 16, one straddling a 16-column block, a set per order; every
# maximum; many blocks; many tiles, two of them empty in the middle of sample 0
CASES = [(1, 1, (4, 4), 1, False, False), (3, 5, (16, 8, 4), 3, False, False),
         (5, 17, (16, 8, 4), 3, True, False), (4, 40, (8, 12, 20), 2, True, True),
         (2, 33, (32, 32, 32, 32), 4, True, True), (67, 20, (16, 8, 4), 3, False, True),
         (3, 300, (16, 8, 4), 3, False, False)]
# single layers: no tanh on the path, so integer operands give exact integers in fp32
INTEGER_CASES = [(3, 5, (16, 8), 3, False, False), (4, 40, (8, 20), 2, True, True)]


def param_len(widths, orders, bias, indep):
    per = sum(a * b + (b if bias else 0) for a, b in zip(widths[:-1], widths[1:]))
    return per * (orders if indep else 1)


@functools.lru_cache(maxsize=None)
def case(key, kind):
    """fp64 tensors that are exact in fp32.  kind "integer": everything from {-2, ..., 2};
    "real": his ~ N(0, 1) / 2, param ~ N(0, 1) / sqrt(d0), go ~ N(0, 1) / sqrt(T).  The mask is
    Bernoulli(0.7) with position 0 of sample 0 live; the last sample's is all zero when B > 1; at T = 300 sample 0 has the
    positions 16..47 masked."""
    B, T, widths, orders, bias, indep = key
    g = torch.Generator().manual_seed(1000 * B + 10 * T + sum(widths) + orders + 2 * bias + indep)
    if kind == "integer":
        r = lambda *s: torch.randint(-2, 3, s, generator=g).double()  # noqa: E731
        hs = ps = gs = 1.0
    else:
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
        hs, ps, gs = 0.5, widths[0] ** -0.5, T ** -0.5
    f32 = lambda t: t.float().double()  # noqa: E731
    mask = (torch.rand(B, T, generator=g) < 0.7).double()
    mask[0, 0] = 1
    if B > 1:
        mask[-1] = 0
    if T == 300:
        mask[0, 16:48] = 0
    return dict(param=f32(r(B, param_len(widths, orders, bias, indep)) * ps),
                his=f32(r(B, T, widths[0]) * hs), mask=mask,
                go=f32(r(B, orders * sum(widths[1:])) * gs))


def compose(param, his, mask, widths, orders, bias, indep):
    """The contract, plainly."""
    outs = []
    for p in range(orders):
        w = param[:, p * (param.shape[1] // orders):] if indep else param
        h, at = his ** (p + 1), 0
        for j in range(1, len(widths)):
            a, b = widths[j - 1], widths[j]
            h = torch.einsum("bta,bac->btc", h, w[:, at:at + a * b].reshape(-1, a, b))
            at += a * b
            if bias:
                h, at = h + w[:, None, at:at + b], at + b
            h = torch.tanh(h) if j + 1 < len(widths) else h
            outs.append(h)
    return (torch.cat(outs, -1) * mask.unsqueeze(-1)).sum(1)


def run(key, cs, fn, dtype, dev, rows=slice(None)):
    """out and the gradients of fn(param, his, mask, widths, orders, bias, order_indep)."""
    t = {n: cs[n][rows].to(dtype).to(dev).clone() for n in cs}
    t["param"].requires_grad_()
    t["his"].requires_grad_()
    out = fn(t["param"], t["his"], t["mask"], *key[2:])
    out.backward(t["go"])
    return dict(out=out.detach(), dhis=t["his"].grad, dparam=t["param"].grad)


@functools.lru_cache(maxsize=None)
def reference(key, kind):
    return run(key, case(key, kind), compose, torch.float64, "cpu")


def ratio(got, want):
    """max |got - want| / (atol + rtol |want|): <= 1 passes."""
    want = want.to(got.device)
    return float(((got.double() - want).abs() / (TOL + TOL * want.abs())).max())
