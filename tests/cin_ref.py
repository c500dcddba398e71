"""Seeded cases and the fp64 reference of the CIN tests."""
import functools

import torch

NAMES = ("out", "dx0", "dxk", "dw", "dbias")
TOL = 1e-5          # rtol = atol: the project's kernel bound

# (B, m, Hk, Hn, D): every minimum; nothing a multiple of 4 or 16, tiles straddle samples,
# ragged last tile; the paper's first layer, 12.5 row tiles; a hidden layer, 33 column tiles;
# every maximum; 65 600 columns, so every slice of the grad_W split holds many tiles
SHAPES = [(1, 1, 1, 1, 1), (5, 5, 5, 17, 10), (2, 39, 39, 200, 10), (33, 26, 128, 128, 16),
          (2, 64, 256, 256, 64), (4100, 3, 4, 16, 16)]
# (shape, bias, xk is x0): the first-layer shapes (Hk = m) also aliased
CASES = [(s, bias, alias) for s in SHAPES for bias in (False, True)
         for alias in ((False, True) if s[1] == s[2] else (False,))]


@functools.lru_cache(maxsize=None)
def case(shape, bias, alias, kind):
    """fp64 tensors that are exact in fp32.  kind "integer": everything, go included, from
    {-2, ..., 2}; "real": N(0, 1) with W / sqrt(Hk m) and go / sqrt(B D) (unscaled, grad_W is
    a long sum that may end near zero, where fp32 cannot meet atol)."""
    B, m, Hk, Hn, D = shape
    g = torch.Generator().manual_seed(sum(p * s for p, s in zip((7, 11, 13, 17, 19), shape))
                                      + 2 * bias + alias)
    if kind == "integer":
        r = lambda *s: torch.randint(-2, 3, s, generator=g).double()  # noqa: E731
        ws = gs = 1.0
    else:
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
        ws, gs = (Hk * m) ** -0.5, (B * D) ** -0.5
    f32 = lambda t: t.float().double()  # noqa: E731
    x0 = f32(r(B, m, D))
    return dict(x0=x0, xk=None if alias else f32(r(B, Hk, D)), w=f32(r(Hn, Hk, m) * ws),
                bias=f32(r(Hn)) if bias else None, go=f32(r(B, Hn, D) * gs))


def compose(x0, xk, w, bias=None):
    """The contract, plainly."""
    out = torch.einsum("hij,bid,bjd->bhd", w, xk, x0)
    return out if bias is None else out + bias[:, None]


def run(cs, fn, dtype, dev, rows=slice(None)):
    """out and the gradients of fn through autograd; xk None: the layer reads x0 twice."""
    t = {n: None if cs[n] is None else cs[n].to(dtype).to(dev).clone() for n in cs}
    for n in ("x0", "xk"):
        t[n] = None if t[n] is None else t[n][rows].contiguous()
    for n in ("x0", "xk", "w", "bias"):
        if t[n] is not None:
            t[n].requires_grad_()
    out = fn(t["x0"], t["x0"] if t["xk"] is None else t["xk"], t["w"], t["bias"])
    out.backward(t["go"][rows].contiguous())
    grad = lambda n: None if t[n] is None else t[n].grad  # noqa: E731
    return dict(out=out.detach(), dx0=grad("x0"), dxk=grad("xk"), dw=grad("w"), dbias=grad("bias"))


@functools.lru_cache(maxsize=None)
def reference(*key):
    return run(case(*key), compose, torch.float64, "cpu")


def ratio(got, want):
    """max |got - want| / (atol + rtol |want|): <= 1 passes."""
    want = want.to(got.device)
    return float(((got.double() - want).abs() / (TOL + TOL * want.abs())).max())
