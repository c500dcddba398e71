"""Seeded cases and the fp64 reference of the multi-head attention tests: a loop
over samples and heads on x[:L] slices, not the masked batched form of ops."""
import functools

import torch

NAMES = ("out", "dq", "dk", "dv")
TOL = 1e-5          # rtol = atol: the project's kernel bound


@functools.lru_cache(maxsize=None)
def case(B, T, heads, head_dim, seed=0):
    """fp64 q, k, v = relu(randn), grad_out = randn, lengths U[0, T], lens[:2] = T, 0."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + heads + head_dim + seed)
    E = heads * head_dim
    r = lambda: torch.randn(B, T, E, generator=g, dtype=torch.float64)  # noqa: E731
    lens = torch.randint(0, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    return dict(q=torch.relu(r()), k=torch.relu(r()), v=torch.relu(r()), go=r(),
                lens=lens.to(torch.int32), heads=heads)


@functools.lru_cache(maxsize=None)
def reference(B, T, heads, head_dim):
    """out and the three gradients in fp64, one (sample, head) at a time."""
    cs = case(B, T, heads, head_dim)
    q, k, v = (cs[n].clone().requires_grad_() for n in "qkv")
    out = torch.zeros_like(q)
    for b in range(B):
        L = int(cs["lens"][b])
        for h in range(heads):
            c = slice(h * head_dim, (h + 1) * head_dim)
            if L:
                p = torch.softmax(q[b, :L, c] @ k[b, :L, c].t() * head_dim ** -0.5, -1)
                out[b, :L, c] = p @ v[b, :L, c]
    out.backward(cs["go"])
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def run(cs, fn, dtype, dev):            # out and the gradients of fn through autograd
    q, k, v = (cs[n].to(dtype).to(dev).requires_grad_() for n in "qkv")
    out = fn(q, k, v, cs["lens"].to(dev), cs["heads"])
    out.backward(cs["go"].to(dtype).to(dev))
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def ratio(got, want):
    """max |got - want| / (atol + rtol |want|): <= 1 passes."""
    want = want.to(got.device)
    return float(((got.double() - want).abs() / (TOL + TOL * want.abs())).max())
