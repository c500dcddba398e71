"""CPU reference of the dense-table Adam, FTRL and AdagradDecay steps
(dr_dense_apply_grouped_ex): the optimizer's _deduplicate_indexed_slices from
the oracle (unique + unsorted_segment_sum, multihash_ref.dedup) and numpy
float32 restatements of the three element updates, one ufunc per rounding --
every operand is a float32 array or scalar, so numpy rounds each operation to
fp32 as the kernels (built without contraction) do.  Tables are updated in
place.  tests/test_dense_opt_ref.py checks the three against float64
restatements before the GPU tests trust them."""
import numpy as np

import multihash_ref

F = np.float32


def adam(orc, w, m, v, idx, val, lr, b1, b2, eps, b1p, b2p):
    """adam.py _apply_sparse_shared on a dense table: every row decays and
    moves, the rows named by idx take the summed gradient.  b1p / b2p are the
    beta powers as they stand; the caller advances them."""
    u, g = multihash_ref.dedup(orc, idx, val)
    lr, b1, b2, eps, b1p, b2p = F(lr), F(b1), F(b2), F(eps), F(b1p), F(b2p)
    alpha = lr * np.sqrt(F(1) - b2p) / (F(1) - b1p)
    mn = m[u] * b1 + g * (F(1) - b1)
    vn = v[u] * b2 + (g * g) * (F(1) - b2)
    wn = w[u] - (mn * alpha) / (np.sqrt(vn) + eps)
    m *= b1                       # nothing added: a -0.0 stays -0.0
    v *= b2
    w -= (m * alpha) / (np.sqrt(v) + eps)
    m[u], v[u], w[u] = mn, vn, wn


def ftrl(orc, w, acc, lin, idx, val, lr, l1, l2, lr_power, l2_shrinkage):
    """ResourceSparseApplyFtrl[V2], elementwise, on the rows named by idx."""
    u, g = multihash_ref.dedup(orc, idx, val)
    if u.size == 0:
        return
    lr, l1, l2, l2s = F(lr), F(l1), F(l2), F(l2_shrinkage)
    x, a, ln = w[u], acc[u], lin[u]
    gu = g + (F(2) * l2s) * x if l2s > 0 else g
    na = a + g * g
    if F(lr_power) == F(-0.5):
        pn, po = np.sqrt(na), np.sqrt(a)
    else:                         # powf: not bit-comparable, see the GPU test
        pn, po = np.power(na, -F(lr_power)), np.power(a, -F(lr_power))
    ln = ln + (gu - ((pn - po) / lr) * x)
    y = pn / lr + F(2) * l2
    w[u] = (np.minimum(np.maximum(ln, -l1), l1) - ln) / y
    lin[u] = ln
    acc[u] = na


def adagrad_decay(orc, w, acc, count, idx, val, lr, decay_step, decay_rate, baseline,
                  global_step):
    """SparseApplyAdagradDecay with one int64 count per row; global_step is
    what the kernel sees (the optimizer's step + 1)."""
    u, g = multihash_ref.dedup(orc, idx, val)
    if u.size == 0:
        return
    lr, rate, base = F(lr), F(decay_rate), F(baseline)
    dec = (np.int64(global_step) // np.int64(decay_step)) > count[u]
    a = acc[u]
    a = np.where(dec[:, None], np.maximum(a * rate, base), a)
    count[u] += dec.astype(np.int64)
    a = a + g * g
    acc[u] = a
    w[u] = w[u] - (lr * g) * (F(1) / np.sqrt(a))
