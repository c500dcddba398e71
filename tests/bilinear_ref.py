"""Seeded cases and the fp64 reference of the bilinear-interaction tests."""
import functools
import itertools

import torch

NAMES = ("out", "dx", "dscale", "dw")
KINDS = ("all", "each", "interaction")
TOL = 1e-5          # rtol = atol: the project's kernel bound

# (B, m, D): every minimum; nothing a multiple of 4 or 16; D two 16-panels and one more, ragged
# last tile; the Criteo shape, two tiles and one sample; every maximum, P = 2016; a long batch,
# so every grad_W slice holds many tiles
SHAPES = [(1, 2, 1), (5, 3, 10), (17, 7, 33), (33, 26, 16), (2, 64, 64), (4100, 4, 16)]
# (shape, kind, scale present)
CASES = [(s, k, a) for s in SHAPES for k in KINDS for a in (False, True)]


@functools.lru_cache(maxsize=None)
def case(shape, kind, scaled, values):
    """fp64 tensors that are exact in fp32.  values "integer": everything from {-2, ..., 2};
    "real": x N(0, 1), W N(0, 1) / sqrt(D), scale uniform [0, 2), go N(0, 1) / sqrt(B m)."""
    B, m, D = shape
    P = m * (m - 1) // 2
    g = torch.Generator().manual_seed(7 * B + 11 * m + 13 * D + 17 * KINDS.index(kind) + scaled)
    if values == "integer":
        r = u = lambda *s: torch.randint(-2, 3, s, generator=g).double()  # noqa: E731
        ws = gs = 1.0
    else:
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
        u = lambda *s: 2 * torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
        ws, gs = D ** -0.5, (B * m) ** -0.5
    f32 = lambda t: t.float().double()  # noqa: E731
    n = {"all": 1, "each": m, "interaction": P}[kind]
    return dict(x=f32(r(B, m, D)), w=f32(r(n, D, D) * ws), scale=f32(u(B, m)) if scaled else None,
                go=f32(r(B, P, D) * gs))


def compose(x, weight, kind="interaction", scale=None):
    """The contract, plainly: one pair at a time, in itertools.combinations' order."""
    v = x if scale is None else x * scale[:, :, None]
    out = []
    for p, (i, j) in enumerate(itertools.combinations(range(x.shape[1]), 2)):
        w = weight[{"all": 0, "each": i, "interaction": p}[kind]]
        out.append((v[:, i] @ w) * v[:, j])
    return torch.stack(out, 1)


def run(cs, kind, fn, dtype, dev, rows=slice(None)):
    """out and the gradients of fn through autograd."""
    t = {n: None if cs[n] is None else cs[n].to(dtype).to(dev).clone() for n in cs}
    for n in ("x", "scale", "go"):
        t[n] = None if t[n] is None else t[n][rows].contiguous()
    for n in ("x", "w", "scale"):
        if t[n] is not None:
            t[n].requires_grad_()
    out = fn(t["x"], t["w"], kind, t["scale"])
    out.backward(t["go"])
    grad = lambda n: None if t[n] is None else t[n].grad  # noqa: E731
    return dict(out=out.detach(), dx=grad("x"), dscale=grad("scale"), dw=grad("w"))


@functools.lru_cache(maxsize=None)
def reference(shape, kind, scaled, values):
    return run(case(shape, kind, scaled, values), kind, compose, torch.float64, "cpu")


def ratio(got, want):
    """max |got - want| / (atol + rtol |want|): <= 1 passes."""
    want = want.to(got.device)
    return float(((got.double() - want).abs() / (TOL + TOL * want.abs())).max())
