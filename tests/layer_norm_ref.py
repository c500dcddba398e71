"""Seeded cases and the fp64 reference of the layer-norm tests."""
import functools

import torch

NAMES = ("out", "dx", "dmask", "dgain", "dbias")
TOL = 1e-5          # rtol = atol: the project's kernel bound


@functools.lru_cache(maxsize=None)
def case(B, D, P, relu, eps, bare):
    """fp64 inputs rounded through fp32: rows N(0,1) U[0.5, 2] + U[-4, 4], gain 1 + 0.5 N, the
    rest N(0,1).  bare: no residual and no mask (P = 1, out [B, D]).  Past 4096 rows go is
    N(0,1) / 256: a column sum over that many N(0,1) terms is of order sqrt(B) while it runs and
    may end near 0, where its fp32 rounding (2^-24 sqrt(B) per add) would pass atol = 1e-5."""
    g = torch.Generator().manual_seed(100000 * B + 100 * D + 10 * P + int(relu))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, 1, generator=g, dtype=torch.float64)  # noqa: E731
    f32 = lambda t: t.float().double()  # noqa: E731
    cs = dict(x=f32(r(B, D) * u(0.5, 2) + u(-4, 4)), gain=f32(1 + 0.5 * r(D)), bias=f32(r(D)),
              residual=None if bare else f32(r(B, D)), mask=None if bare else f32(r(B, P, D)),
              go=f32((r(B, D) if bare else r(B, P, D)) / (256 if B > 4096 else 1)), eps=eps,
              relu=relu)
    return cs


def compose(x, gain, bias, eps, residual=None, mask=None, relu=False):
    """The contract, plainly."""
    s = x if residual is None else x + residual
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    a = gain * (s - mean) / torch.sqrt(var + eps) + bias
    a = torch.relu(a) if relu else a
    return a if mask is None else a[:, None, :] * mask


def run(cs, fn, dtype, dev):
    """out and the gradients of fn through autograd; the residual's gradient must be x's."""
    t = {n: None if cs[n] is None else cs[n].to(dtype).to(dev).clone().requires_grad_()
         for n in ("x", "gain", "bias", "residual", "mask")}
    out = fn(t["x"], t["gain"], t["bias"], cs["eps"], t["residual"], t["mask"], cs["relu"])
    out.backward(cs["go"].to(dtype).to(dev))
    if t["residual"] is not None:
        assert torch.equal(t["residual"].grad, t["x"].grad)
    res = dict(out=out.detach(), dx=t["x"].grad, dgain=t["gain"].grad, dbias=t["bias"].grad)
    if t["mask"] is not None:
        res["dmask"] = t["mask"].grad
    return res


@functools.lru_cache(maxsize=None)
def reference(*key):
    return run(case(*key), compose, torch.float64, "cpu")


def ratio(got, want):
    """max |got - want| / (atol + rtol |want|): <= 1 passes."""
    want = want.to(got.device)
    return float(((got.double() - want).abs() / (TOL + TOL * want.abs())).max())
