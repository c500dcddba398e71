"""Seeded cases and the fp64 reference of the gate-mix tests."""
import functools

import torch

NAMES = ("out", "gates", "dz", "dh")
TOL = 1e-5          # rtol = atol: the project's kernel bound


@functools.lru_cache(maxsize=None)
def case(B, K, E, H, ple):
    """fp64 z = 2 randn, h and go = randn, each rounded through fp32.  ple: task k sees expert
    k % E, every task but task 0 also expert E - 1, and task 0 expert 0 only."""
    g = torch.Generator().manual_seed(100000 * B + 1000 * K + 100 * E + H + int(ple))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    select = None
    if ple:
        select = torch.zeros(K, E, dtype=torch.bool)
        for k in range(K):
            select[k, k % E] = True
            select[k, E - 1] |= k > 0
    return dict(z=(r(B, K, E) * 2).float().double(), h=r(B, E, H), go=r(B, K, H), select=select)


@functools.lru_cache(maxsize=None)
def reference(B, K, E, H, ple):
    """out, gates and the two gradients of the fp64 torch composition."""
    cs = case(B, K, E, H, ple)
    z, h = cs["z"].clone().requires_grad_(), cs["h"].clone().requires_grad_()
    zm = z if cs["select"] is None else z.masked_fill(~cs["select"], float("-inf"))
    gates = torch.softmax(zm, -1)
    out = gates @ h
    out.backward(cs["go"])
    return dict(out=out.detach(), gates=gates.detach(), dz=z.grad, dh=h.grad)


def run(cs, fn, dtype, dev):            # out and the gradients of fn through autograd
    z, h = (cs[n].to(dtype).to(dev).requires_grad_() for n in "zh")
    out = fn(z, h, cs["select"])
    out.backward(cs["go"].to(dtype).to(dev))
    return dict(out=out.detach(), dz=z.grad, dh=h.grad)


def ratio(got, want):
    """max |got - want| / (atol + rtol |want|): <= 1 passes."""
    want = want.to(got.device)
    return float(((got.double() - want).abs() / (TOL + TOL * want.abs())).max())
