"""The float32 reference of the dense Adam / FTRL / AdagradDecay steps
(tests/dense_opt_ref.py) against the float64 restatements the older GPU tests
use (test_gpu_dtypes._adam_ref / _ftrl_ref, and the AdagradDecay loop of
test_gpu_async_decay.test_dense_table_adagrad_decay_and_adam_async, repeated
here): a few steps agree to fp32 rounding.  No GPU."""
import numpy as np

import dense_opt_ref as ref
from test_gpu_dtypes import _adam_ref, _ftrl_ref

R, D, N = 23, 6, 40


def _case(seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((R, D)).astype(np.float32)
    steps = []
    for _ in range(4):
        idx = rng.integers(0, R - 3, N).astype(np.int64)      # repeats; three rows never named
        idx[5] = -1                                           # a skipped position
        g = rng.standard_normal((N, D)).astype(np.float32)
        steps.append((idx, g))
    return w, steps


def _summed(idx, g):
    keep = idx >= 0
    u, inv = np.unique(idx[keep], return_inverse=True)
    gs = np.zeros((u.size, g.shape[1]))
    np.add.at(gs, inv, g[keep].astype(np.float64))
    return u, gs


def test_adam_agrees_with_the_float64_reference(orc):
    w0, steps = _case(1)
    w, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
    w64, m64, v64 = w0.astype(np.float64), np.zeros((R, D)), np.zeros((R, D))
    b1p, b2p = np.float32(0.9), np.float32(0.999)
    for idx, g in steps:
        prev = w.copy()
        ref.adam(orc, w, m, v, idx, g, 0.01, 0.9, 0.999, 1e-8, b1p, b2p)
        keep = idx >= 0
        w64, m64, v64 = _adam_ref(w64, m64, v64, idx[keep], g[keep].astype(np.float64), 0.01, 0.9,
                                  0.999, 1e-8, float(b1p), float(b2p))
        b1p, b2p = b1p * np.float32(0.9), b2p * np.float32(0.999)
    assert w.dtype == m.dtype == v.dtype == np.float32
    np.testing.assert_allclose(w, w64, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m, m64, rtol=1e-5, atol=1e-7)
    # (1 - beta2) in fp32 is 1.0f - 0.999f = 0.0010000467 (adam.py computes it
    # in the variable's dtype), 4.7e-5 above the float64 0.001: v carries it
    np.testing.assert_allclose(v, v64, rtol=6e-5, atol=1e-7)
    # non-lazy: a row named before the last step and not in it still moved there
    idx, _ = steps[-1]
    earlier = np.unique(np.concatenate([i[i >= 0] for i, _ in steps[:-1]]))
    late = np.setdiff1d(earlier, idx)
    assert late.size and (w[late] != prev[late]).any(1).all()
    assert np.array_equal(w[R - 3:], w0[R - 3:])              # m == 0: the update is 0


def test_adam_keeps_a_negative_zero_m_on_an_unnamed_row(orc):
    w = np.ones((3, 2), np.float32)
    m = np.full((3, 2), -0.0, np.float32)
    v = np.ones((3, 2), np.float32)
    ref.adam(orc, w, m, v, np.array([1], np.int64), np.ones((1, 2), np.float32), 0.01, 0.9,
             0.999, 1e-8, 0.9, 0.999)
    assert np.signbit(m[0]).all() and np.signbit(m[2]).all() and not np.signbit(m[1]).any()


def test_ftrl_agrees_with_the_float64_reference(orc):
    for lr_power, shrink in ((-0.5, 0.0), (-0.5, 0.05), (-0.6, 0.05)):
        w0, steps = _case(2)
        w, acc, lin = w0.copy(), np.full_like(w0, 0.1), np.zeros_like(w0)
        w64, a64, l64 = w0.astype(np.float64), np.full((R, D), 0.1), np.zeros((R, D))
        for idx, g in steps:
            ref.ftrl(orc, w, acc, lin, idx, g, 0.05, 0.01, 0.02, lr_power, shrink)
            u, gs = _summed(idx, g)
            w64, a64, l64 = _ftrl_ref(w64, a64, l64, u, gs, 0.05, 0.01, 0.02, lr_power, shrink)
        assert w.dtype == acc.dtype == lin.dtype == np.float32
        np.testing.assert_allclose(w, w64, rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(acc, a64, rtol=1e-5)
        np.testing.assert_allclose(lin, l64, rtol=1e-4, atol=1e-5)
        assert np.array_equal(w[R - 3:], w0[R - 3:])          # lazy: unnamed rows stay


def test_adagrad_decay_agrees_with_the_float64_reference(orc):
    w0, steps = _case(3)
    w, acc, cnt = w0.copy(), np.full_like(w0, 0.1), np.zeros(R, np.int64)
    w64, a64, c64 = w0.astype(np.float64), np.full((R, D), 0.1), np.zeros(R, np.int64)
    for step, (idx, g) in enumerate(steps):
        gs = step + 1
        ref.adagrad_decay(orc, w, acc, cnt, idx, g, 0.2, 2, 0.5, 0.1, gs)
        u, gsum = _summed(idx, g)
        for j, r in enumerate(u):
            if gs // 2 > c64[r]:
                a64[r] = np.maximum(a64[r] * 0.5, 0.1)
                c64[r] += 1
            a64[r] = a64[r] + gsum[j] ** 2
            w64[r] = w64[r] - 0.2 * gsum[j] / np.sqrt(a64[r])
    assert np.array_equal(cnt, c64) and cnt.max() == 2 and cnt.min() == 0
    np.testing.assert_allclose(w, w64, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(acc, a64, rtol=1e-5)
