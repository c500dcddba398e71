"""Dense Adam, FTRL and AdagradDecay through dr_dense_apply_grouped_ex on the
GPU, against tests/dense_opt_ref.py (the oracle's unique + unsorted segment
sum, then float32 numpy restatements of the three element updates), through
the C entry and through the optimizers.  Comparisons are bit equality except
FTRL with lr_power != -0.5 (powf), which is compared with the float64
reference at the tolerance test_dense_adam_and_ftrl uses.

Shapes are those of tests/test_gpu_dense_apply.py (R = 7 rows with n = 600
positions, widths 1 .. 520, every row shape in one call, 33 tables, capacity
64 with device counts 0 / 1 / 37 / 64) plus, for Adam's sweep over the rows
nobody names, row counts on both sides of a bitmap word (1, 31, 32, 33, 65).

FTRL's l1 = 30000 in the order-sensitive case: the gradients there are scaled
by 2^[-12, 12] and a row sums ~86 of them, so |linear| runs from far below to
far above it and both branches of the clip are taken at every width, the 7
elements of D = 1 included (asserted)."""
import numpy as np
import pytest
import torch

import dense_opt_ref as ref
from test_gpu_dense_apply import ALL_SHAPE_DIMS, order_case
from test_gpu_dtypes import _ftrl_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ADAM, ADAM_ASYNC, FTRL, DECAY = 2, 3, 5, 6
F = np.float32
LR, B1, B2, EPS = 0.05, 0.9, 0.999, 1e-8
OPTS = {
    "adam": (ADAM, {}),
    "ftrl": (FTRL, dict(l1=0.01, l2=0.02, lr_power=-0.5, l2_shrinkage=0.0)),
    "ftrl_v2": (FTRL, dict(l1=0.01, l2=0.02, lr_power=-0.5, l2_shrinkage=0.05)),
    "decay": (DECAY, dict(decay_rate=0.5, decay_baseline=0.1, decay_step=2)),
}


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    deeprec_amd.load()
    deeprec_amd.set_validate(True)
    assert torch.cuda.is_available()
    return deeprec_amd


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), device=DEV, dtype=dtype)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.dtype == np.int64:
        return a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    """Bit equality (NaN payloads and zero signs included; int64 by value)."""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


class Tab(object):
    """One table's state on the device and its reference twin on the host."""

    def __init__(self, w, code):
        w = np.array(w, np.float32)
        self.code = code
        self.h = [w.copy()]
        if code == ADAM:
            self.h += [np.zeros_like(w), np.zeros_like(w)]
            self.b1p, self.b2p = F(B1), F(B2)
        elif code == FTRL:
            self.h += [np.full_like(w, 0.1), np.zeros_like(w)]
        else:
            self.h += [np.full_like(w, 0.1), np.zeros(w.shape[0], np.int64)]
        self.w, self.s1, self.s2 = [T(x.copy()) for x in self.h]
        self.pw = T(np.array([B1, B2], np.float32)) if code == ADAM else None

    def state(self):
        return [t.clone() for t in (self.w, self.s1, self.s2)]

    def ref_step(self, orc, idx, g, kw, lr=LR, gs=1):
        w, s1, s2 = self.h
        if self.code == ADAM:
            ref.adam(orc, w, s1, s2, idx, g, lr, B1, B2, EPS, self.b1p, self.b2p)
        elif self.code == FTRL:
            ref.ftrl(orc, w, s1, s2, idx, g, lr, kw["l1"], kw["l2"], kw["lr_power"],
                     kw["l2_shrinkage"])
        else:
            ref.adagrad_decay(orc, w, s1, s2, idx, g, lr, kw["decay_step"], kw["decay_rate"],
                              kw["decay_baseline"], gs)

    def advance(self):
        """What the optimizer's _finish does: the entry leaves Adam's powers."""
        if self.code == ADAM:
            assert same(self.pw, np.array([self.b1p, self.b2p], np.float32))
            self.pw.mul_(T(np.array([B1, B2], np.float32)))
            self.b1p, self.b2p = self.b1p * F(B1), self.b2p * F(B2)

    def check(self, tag):
        for k, (d, h) in enumerate(zip((self.w, self.s1, self.s2), self.h)):
            assert same(d, h), (tag, k)


def c_apply(dr, code, items, kw, lr=LR, gs=1):
    """items: [(Tab, grad [n, D] device, idx [n] device, n_dev device or None)]."""
    from deeprec_amd._lib import (DrDenseApplyDesc, DrDenseApplyOpts, lib, ptr, stream_handle,
                                  workspace)
    import ctypes as C
    descs = (DrDenseApplyDesc * max(len(items), 1))()
    for d, (tab, g, i, n_dev) in zip(descs, items):
        d.table, d.rows, d.dim = tab.w.data_ptr(), tab.w.shape[0], tab.w.shape[1]
        d.slot1, d.slot2, d.powers = ptr(tab.s1), ptr(tab.s2), ptr(tab.pw)
        d.grad, d.idx, d.n, d.n_dev = ptr(g), ptr(i), i.numel(), ptr(n_dev)
    opts = DrDenseApplyOpts(global_step=gs, **kw)
    wsb = lib().dr_dense_apply_grouped_ex_workspace_size(code, descs, len(items))
    ws = workspace(wsb, DEV)
    rc = lib().dr_dense_apply_grouped_ex(code, descs, len(items), lr, B1, B2, EPS, C.byref(opts),
                                         ptr(ws), wsb, stream_handle(DEV))
    assert rc == 0, lib().dr_last_error()


# ---------------------------------------------------------------------------
# 1. the sum of a run is one serial chain in ascending position order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 4, 6, 16, 128, 200, 520])
@pytest.mark.parametrize("name", ["adam", "ftrl", "ftrl_v2", "decay"])
def test_order_sensitive_sums(dr, orc, name, D):
    code, kw = OPTS[name]
    if code == FTRL:
        kw = dict(kw, l1=30000.0)
    idx, g = order_case(D)
    rng = np.random.default_rng(7)
    tab = Tab(rng.standard_normal((7, D)), code)
    for step in range(2):
        gs = (g * F(1 + step)).astype(np.float32)
        c_apply(dr, code, [(tab, T(gs), T(idx), None)], kw, gs=step + 1)
        tab.ref_step(orc, idx, gs, kw, gs=step + 1)
        tab.advance()
        dr.status_check()
        tab.check((name, D, step))
        if code == FTRL:              # both branches of the clip
            assert (tab.h[0] == 0).any() and (tab.h[0] != 0).any(), (D, step)
        if code == DECAY:             # global steps 1 and 2 at decay_step 2: the second decays
            assert np.array_equal(tab.h[2], np.full(7, step, np.int64)), (D, step)


# ---------------------------------------------------------------------------
# 2. dense Adam moves the rows nobody names
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 6])
@pytest.mark.parametrize("R", [1, 31, 32, 33, 65])
def test_adam_moves_the_rows_nobody_names(dr, orc, R, D):
    rng = np.random.default_rng(100 * R + D)
    tab = Tab(rng.standard_normal((R, D)), ADAM)
    tab.h[1][:] = (rng.standard_normal((R, D)) * 0.1).astype(np.float32)   # m, v non-zero
    tab.h[2][:] = rng.uniform(0.1, 1.0, (R, D)).astype(np.float32)
    mid = R // 2
    if R >= 3:                        # an unnamed row's -0.0 m keeps its sign
        tab.h[1][mid] = -0.0
    tab.s1, tab.s2 = T(tab.h[1].copy()), T(tab.h[2].copy())
    n = 24
    for step in range(4):
        pool = np.array([0, R - 1], np.int64) if step == 0 else np.arange(R, dtype=np.int64)
        idx = rng.choice(pool, n).astype(np.int64)
        idx[:2] = (0, R - 1)
        g = rng.standard_normal((n, D)).astype(np.float32)
        count = 0 if step == 2 else n   # step 2: N == 0, every row still decays and moves
        before = tab.h[0].copy()
        unnamed = np.ones(R, bool)
        unnamed[idx[:count]] = False
        live = unnamed & (tab.h[1] != 0).any(1)    # (a zero m leaves its row where it is)
        c_apply(dr, ADAM, [(tab, T(g), T(idx), T([count], torch.int64))], {}, lr=0.01)
        tab.ref_step(orc, idx[:count], g[:count], {}, lr=0.01)
        tab.advance()
        dr.status_check()
        tab.check((R, D, step))
        if step == 0 and R >= 3:
            assert unnamed[mid] and np.signbit(tab.s1[mid].cpu().numpy()).all()
        assert (bits(tab.w) != bits(before)).any(1)[live].all(), (R, D, step)
        assert step != 2 or live.sum() >= R - 1


# ---------------------------------------------------------------------------
# 3. table layouts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adam", "ftrl_v2", "decay"])
def test_tables_of_every_row_shape_in_one_call(dr, orc, name):
    """One call over tables of every width class equals each table applied
    alone (and the reference).  The last table is 256 wide with a gradient
    block that is only 4-byte aligned (the scalar layout at a 4-wide width)."""
    code, kw = OPTS[name]
    rng = np.random.default_rng(53)
    order = rng.permutation(len(ALL_SHAPE_DIMS))
    items, alone = [], []
    for j in order:
        D = ALL_SHAPE_DIMS[j]
        R, n = 6, 37
        idx = rng.integers(-1, R, n).astype(np.int64)
        g = rng.standard_normal((n, D)).astype(np.float32)
        w = rng.standard_normal((R, D)).astype(np.float32)
        if j == len(ALL_SHAPE_DIMS) - 1:
            flat = torch.zeros(n * D + 1, dtype=torch.float32, device=DEV)
            gd = flat[1:].view(n, D)
            gd.copy_(T(g))
            assert gd.data_ptr() % 16 == 4
        else:
            gd = T(g)
        items.append((Tab(w, code), gd, T(idx), None))
        alone.append((Tab(w, code), gd, T(idx), None))
        items[-1][0].ref_step(orc, idx, g, kw, gs=2)
    c_apply(dr, code, items, kw, gs=2)
    for it in alone:
        c_apply(dr, code, [it], kw, gs=2)
    dr.status_check()
    for (tab, _, _, _), (one, _, _, _), j in zip(items, alone, order):
        D = ALL_SHAPE_DIMS[j]
        assert all(same(a, b) for a, b in zip(tab.state(), one.state())), D
        tab.check((name, D))


def test_33_adam_tables_in_one_call(dr, orc):
    """Two launch groups of one row shape: the second group's bitmap is the
    first's memory (cleared per group), its tables' words start again at 0."""
    rng = np.random.default_rng(54)
    items = []
    for t in range(33):
        R, D = 3 + (t * 7) % 41, 4
        n = 0 if t == 13 else int(rng.integers(1, 50))
        idx = rng.integers(-1, R, n).astype(np.int64)
        g = rng.standard_normal((n, D)).astype(np.float32)
        tab = Tab(rng.standard_normal((R, D)), ADAM)
        tab.h[1][:] = rng.standard_normal((R, D)).astype(np.float32)   # m, v non-zero: rows move
        tab.h[2][:] = rng.uniform(0.1, 1.0, (R, D)).astype(np.float32)
        tab.s1, tab.s2 = T(tab.h[1].copy()), T(tab.h[2].copy())
        items.append((tab, T(g), T(idx), None))
        tab.ref_step(orc, idx, g, {}, lr=0.01)
    c_apply(dr, ADAM, items, {}, lr=0.01)
    dr.status_check()
    for t, (tab, _, _, _) in enumerate(items):
        tab.check(t)


# ---------------------------------------------------------------------------
# 4. counts and indices
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adam", "ftrl", "decay"])
@pytest.mark.parametrize("count", [0, 1, 37, 64])
def test_device_count(dr, orc, name, count):
    code, kw = OPTS[name]
    rng = np.random.default_rng(31)
    R, D, cap = 9, 4, 64
    idx = rng.integers(0, R, cap).astype(np.int64)
    idx[::5] = -1                     # skipped positions inside the count
    g = rng.standard_normal((cap, D)).astype(np.float32)
    idx_d, g_d = idx.copy(), g.copy()
    idx_d[count:] = np.int64(1) << 40  # past the count: far out of range, NaN values
    g_d[count:] = np.nan
    tab = Tab(rng.standard_normal((R, D)), code)
    before = tab.state()
    c_apply(dr, code, [(tab, T(g_d), T(idx_d), T([count], torch.int64))], kw, gs=4)
    dr.status_check()                 # nothing past the count was looked at
    tab.ref_step(orc, idx[:count], g[:count], kw, gs=4)
    tab.check((name, count))
    if count == 0 and code != ADAM:
        assert all(same(a, b) for a, b in zip(tab.state(), before))
    if count == 0 and code == ADAM:   # m = v = 0: w - 0 / (0 + eps)
        assert same(tab.w, before[0])


@pytest.mark.parametrize("name", ["adam", "ftrl", "decay"])
def test_out_of_range_index_is_skipped_and_latches(dr, orc, name):
    from deeprec_amd._lib import InvalidArgumentError
    code, kw = OPTS[name]
    rng = np.random.default_rng(41)
    R, D, n = 6, 4, 20
    idx = rng.integers(0, R, n).astype(np.int64)
    idx[7] = R
    g = rng.standard_normal((n, D)).astype(np.float32)
    tab = Tab(rng.standard_normal((R, D)), code)
    dr.status_check()
    c_apply(dr, code, [(tab, T(g), T(idx), None)], kw)
    with pytest.raises(InvalidArgumentError):
        dr.status_check()
    dr.status_check()                 # raised once, clear afterwards
    keep = np.arange(n) != 7
    tab.ref_step(orc, idx[keep], g[keep], kw)
    tab.check(name)


# ---------------------------------------------------------------------------
# 5. through apply_gradients
# ---------------------------------------------------------------------------
def make_opt(dr, name, lr_power=-0.5):
    if name == "adam":
        return dr.AdamOptimizer(0.01, B1, B2, EPS)
    if name == "decay":
        return dr.AdagradDecayOptimizer(LR, initial_accumulator_value=0.1,
                                        accumulator_decay_step=2, accumulator_decay_rate=0.5)
    return dr.FtrlOptimizer(LR, learning_rate_power=lr_power, initial_accumulator_value=0.1,
                            l1_regularization_strength=0.01, l2_regularization_strength=0.02,
                            l2_shrinkage_regularization_strength=0.05)


def opt_state(opt, name, tab):
    return opt._dense_mv[id(tab)] if name == "adam" else opt._dense[id(tab)]


def slices(rng, R, D):
    """Two pending slices, the second with a device count and garbage past it."""
    count = int(rng.integers(0, 21))
    i1 = rng.integers(0, R, 30).astype(np.int64)
    g1 = rng.standard_normal((30, D)).astype(np.float32)
    i2 = rng.integers(0, R, 20).astype(np.int64)
    g2 = rng.standard_normal((20, D)).astype(np.float32)
    i2d, g2d = i2.copy(), g2.copy()
    i2d[count:] = np.int64(1) << 40
    g2d[count:] = np.nan
    return (i1, g1, i2d, g2d, count,
            np.concatenate([i1, i2[:count]]), np.concatenate([g1, g2[:count]]))


@pytest.mark.parametrize("name", ["adam", "ftrl_v2", "decay"])
def test_five_apply_gradients_steps_equal_the_reference(dr, orc, name):
    code, kw = OPTS[name]
    rng = np.random.default_rng(71)
    shapes = [(12, 6), (9, 16)]
    twins = [Tab(rng.standard_normal(s), code) for s in shapes]     # host reference only
    tabs = [dr.DenseTable(T(t.h[0].copy())) for t in twins]
    opt = make_opt(dr, name)
    lr = 0.01 if name == "adam" else LR
    for step in range(5):
        i1, g1, i2d, g2d, count, idx, g = slices(rng, *shapes[0])
        tabs[0].pending_grads.append(dr.IndexedSlices(T(g1), T(i1)))
        tabs[0].pending_grads.append(dr.IndexedSlices(T(g2d), T(i2d), T([count], torch.int64)))
        twins[0].ref_step(orc, idx, g, kw, lr=lr, gs=step + 1)
        ib = rng.integers(0, shapes[1][0], 25).astype(np.int64)
        gb = rng.standard_normal((25, shapes[1][1])).astype(np.float32)
        tabs[1].pending_grads.append(dr.IndexedSlices(T(gb), T(ib)))
        twins[1].ref_step(orc, ib, gb, kw, lr=lr, gs=step + 1)
        opt.apply_gradients(tabs, global_step=step)
        dr.status_check()
        for tab, twin in zip(tabs, twins):
            if code == ADAM:
                twin.b1p, twin.b2p = twin.b1p * F(B1), twin.b2p * F(B2)
            s1, s2 = opt_state(opt, name, tab)
            assert same(tab.weight, twin.h[0]), (name, step)
            assert same(s1, twin.h[1]) and same(s2, twin.h[2]), (name, step)
    if code == DECAY:
        assert twins[0].h[2].max() == 2


def test_five_ftrl_powf_steps_are_close_to_the_float64_reference(dr):
    """lr_power = -0.6 takes powf, whose device and host roundings differ:
    the float64 restatement at test_dense_adam_and_ftrl's tolerance."""
    rng = np.random.default_rng(72)
    R, D = 12, 6
    w0 = rng.standard_normal((R, D)).astype(np.float32)
    tab = dr.DenseTable(T(w0.copy()))
    opt = make_opt(dr, "ftrl", lr_power=-0.6)
    w, acc, lin = w0.astype(np.float64), np.full((R, D), 0.1), np.zeros((R, D))
    for step in range(5):
        i1, g1, i2d, g2d, count, idx, g = slices(rng, R, D)
        tab.pending_grads.append(dr.IndexedSlices(T(g1), T(i1)))
        tab.pending_grads.append(dr.IndexedSlices(T(g2d), T(i2d), T([count], torch.int64)))
        opt.apply_gradients([tab], global_step=step)
        dr.status_check()
        u, inv = np.unique(idx, return_inverse=True)
        gu = np.zeros((u.size, D))
        np.add.at(gu, inv, g.astype(np.float64))
        w, acc, lin = _ftrl_ref(w, acc, lin, u, gu, LR, 0.01, 0.02, -0.6, 0.05)
    np.testing.assert_allclose(tab.weight.cpu().numpy(), w, rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------------------
# 6. on a fully named table dense Adam is AdamAsync (the element pinned to the EV kernels)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 6])
def test_adam_equals_adam_async_on_fully_named_tables(dr, D):
    rng = np.random.default_rng(61 + D)
    R = 11
    w0 = rng.standard_normal((R, D)).astype(np.float32)
    t_adam, t_async = dr.DenseTable(T(w0.copy())), dr.DenseTable(T(w0.copy()))
    o_adam = dr.AdamOptimizer(0.01, B1, B2, EPS)
    o_async = dr.AdamAsyncOptimizer(0.01, B1, B2, EPS)
    assert o_async._power(t_async) == o_adam._device_powers(torch.device(DEV)).tolist()
    for step in range(3):
        idx = rng.permutation(R).astype(np.int64)             # every row named once
        g = (rng.standard_normal((R, D)) * 0.3).astype(np.float32)
        for var in (t_adam, t_async):
            var.pending_grads.append(dr.IndexedSlices(T(g), T(idx)))
        o_adam.apply_gradients([t_adam], global_step=step)
        o_async.apply_gradients([t_async], global_step=step)
        dr.status_check()
        assert same(t_adam.weight, t_async.weight), step
        for a, b in zip(o_adam._dense_mv[id(t_adam)], o_async._dense_mv[id(t_async)]):
            assert same(a, b), step
        assert o_async._power(t_async) == o_adam._device_powers(torch.device(DEV)).tolist()
    assert not same(t_adam.weight, w0)


# ---------------------------------------------------------------------------
# 7. under stream capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adam", "ftrl_v2"])
def test_captured_apply_replays_with_new_slices(dr, name):
    """One captured apply_gradients replayed three times against an eager
    twin.  (With DR_DENSE_APPLY=torch the capture raises: the torch path reads
    the count on the host.)"""
    rng = np.random.default_rng(91)
    R, D, cap = 10, 16, 48
    w0 = rng.standard_normal((R, D)).astype(np.float32)
    tab, twin = dr.DenseTable(T(w0.copy())), dr.DenseTable(T(w0.copy()))
    opt, opt2 = make_opt(dr, name), make_opt(dr, name)
    if name == "adam":
        opt.prepare(DEV)
    vals = torch.zeros((cap, D), dtype=torch.float32, device=DEV)
    idxs = torch.zeros(cap, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)

    def fill(count):
        vals.copy_(T(rng.standard_normal((cap, D)).astype(np.float32)))
        idxs.copy_(T(rng.integers(0, R, cap).astype(np.int64)))
        cnt.fill_(count)

    def eager(step):
        twin.pending_grads.append(dr.IndexedSlices(vals.clone(), idxs.clone(), cnt.clone()))
        opt2.apply_gradients([twin], global_step=step)

    def agree(tag):
        assert same(tab.weight, twin.weight), tag
        for a, b in zip(opt_state(opt, name, tab), opt_state(opt2, name, twin)):
            assert same(a, b), tag

    # one eager step first: the slots exist before the capture
    fill(cap)
    tab.pending_grads.append(dr.IndexedSlices(vals, idxs, cnt))
    opt.apply_gradients([tab], global_step=0)
    eager(0)
    dr.status_check()
    agree("eager")
    assert not same(tab.weight, w0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    tab.pending_grads.append(dr.IndexedSlices(vals, idxs, cnt))
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):     # (capturing runs nothing)
        opt.apply_gradients([tab], global_step=1)
    for step, count in enumerate((31, 0, cap)):
        fill(count)
        graph.replay()
        torch.cuda.synchronize()
        eager(1 + step)
        dr.status_check()
        agree(count)
