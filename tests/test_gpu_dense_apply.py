"""The grouped dense-table apply (dr_dense_apply_grouped) on the GPU: dedup and
update on the device against the CPU oracle's unique + unsorted_segment_sum +
dense applies (tests/multihash_ref.py), through the C entry and through the
optimizers.  Every comparison is bit equality.

Shapes are the smallest at which each piece can go wrong: R = 7 rows with
n = 600 positions (runs of ~86, many walk batches, several blocks), row widths
1, 4, 6, 16, 128, 200, 520 (scalar and 4-wide layouts, one and several lanes
per row, one and several column chunks per lane), one call over tables of
every row shape, 33 tables of mixed width and 33 of one width (more than a
launch group), capacity 64 with device counts 0, 1, 37, 64."""
import ctypes as C

import numpy as np
import pytest
import torch

import multihash_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SGD, ADAGRAD, ADAM_ASYNC, RMSPROP = 0, 1, 3, 4
INVALID_ARGUMENT = 3
LR = 0.05
_N = [0]


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
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    """Bit equality of two fp32 arrays (NaN payloads and zero signs included)."""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


class Tab(object):
    """One descriptor's device state: table, slots, powers."""

    def __init__(self, w, opt, acc0=0.1):
        self.w = T(np.array(w, np.float32))
        self.s1 = self.s2 = self.pw = None
        if opt == ADAGRAD:
            self.s1 = torch.full_like(self.w, acc0)
        if opt in (ADAM_ASYNC, RMSPROP):
            self.s1, self.s2 = torch.zeros_like(self.w), torch.zeros_like(self.w)
        if opt == ADAM_ASYNC:
            self.pw = T(np.array([0.9, 0.999], np.float32))

    def state(self):
        return [t.clone() for t in (self.w, self.s1, self.s2, self.pw) if t is not None]


def c_apply(dr, opt, items, lr=LR):
    """items: [(Tab, grad [n, D] device, idx [n] device, n_dev device or None)]."""
    from deeprec_amd._lib import DrDenseApplyDesc, lib, ptr, stream_handle, workspace
    descs = (DrDenseApplyDesc * max(len(items), 1))()
    for d, (tab, g, i, n_dev) in zip(descs, items):
        d.table, d.rows, d.dim = tab.w.data_ptr(), tab.w.shape[0], tab.w.shape[1]
        d.slot1, d.slot2, d.powers = ptr(tab.s1), ptr(tab.s2), ptr(tab.pw)
        d.grad, d.idx, d.n, d.n_dev = ptr(g), ptr(i), i.numel(), ptr(n_dev)
    wsb = lib().dr_dense_apply_grouped_workspace_size(descs, len(items))
    ws = workspace(wsb, DEV)
    rc = lib().dr_dense_apply_grouped(opt, descs, len(items), lr, 0.9, 0.999, 1e-8, ptr(ws), wsb,
                                      stream_handle(DEV))
    assert rc == 0, lib().dr_last_error()


def ref_apply(orc, opt, w, acc, idx, val, lr=LR):
    if opt == SGD:
        ref.apply_sgd(orc, w, lr, idx, val)
    else:
        ref.apply_adagrad(orc, w, acc, lr, idx, val)


# ---------------------------------------------------------------------------
# 1. the sum of a run is one serial chain in ascending position order
# ---------------------------------------------------------------------------
_ORDER = {}


def order_case(D):
    if D not in _ORDER:
        rng = np.random.default_rng(2101)
        n = 600
        idx = rng.integers(0, 7, n).astype(np.int64)
        g = (rng.standard_normal((n, D)) * np.exp2(rng.integers(-12, 13, (n, 1)))).astype(np.float32)
        _ORDER[D] = (idx, g)
    return _ORDER[D]


@pytest.mark.parametrize("D", [1, 4, 6, 16, 128, 200, 520])
@pytest.mark.parametrize("opt", [SGD, ADAGRAD])
def test_order_sensitive_sums(dr, orc, opt, D):
    idx, g = order_case(D)
    # the inputs tell the orders apart: ascending and descending serial sums
    # (and the fp64 sum rounded once) differ in bits
    u, up = ref.dedup(orc, idx, g)
    u2, down = ref.dedup(orc, idx[::-1].copy(), g[::-1].copy())
    down = down[[list(u2).index(r) for r in u]]
    assert (bits(up) != bits(down)).sum() > up.size // 2
    exact = np.stack([g[idx == r].astype(np.float64).sum(0) for r in u])
    assert (bits(up) != bits(exact.astype(np.float32))).sum() > up.size // 2
    rng = np.random.default_rng(7)
    w = rng.standard_normal((7, D)).astype(np.float32)
    acc = np.full((7, D), 0.1, np.float32)
    tab = Tab(w, opt)
    for step in range(3):             # the accumulator carries
        gs = (g * np.float32(1 + step)).astype(np.float32)
        c_apply(dr, opt, [(tab, T(gs), T(idx), None)])
        ref_apply(orc, opt, w, acc, idx, gs)
        dr.status_check()
        assert same(tab.w, w), (opt, D, step)
        if opt == ADAGRAD:
            assert same(tab.s1, acc), (D, step)


# ---------------------------------------------------------------------------
# 2. edge cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [SGD, ADAGRAD])
@pytest.mark.parametrize("D", [4, 6])
def test_edge_cases(dr, orc, opt, D):
    rng = np.random.default_rng(11 + D)
    R, n = 40, 33
    g = rng.standard_normal((n, D)).astype(np.float32)
    cases = {
        "one row": np.full(n, 5, np.int64),
        "distinct": rng.permutation(R)[:n].astype(np.int64),
        "skips": np.where(np.arange(n) % 3 == 1, -1, rng.integers(0, 4, n)).astype(np.int64),
        "all skipped": np.full(n, -1, np.int64),
    }
    for name, idx in cases.items():
        w = rng.standard_normal((R, D)).astype(np.float32)
        acc = np.full((R, D), 0.1, np.float32)
        tab = Tab(w, opt)
        c_apply(dr, opt, [(tab, T(g), T(idx), None)])
        ref_apply(orc, opt, w, acc, idx, g)
        dr.status_check()
        assert same(tab.w, w), name
        if opt == ADAGRAD:
            assert same(tab.s1, acc), name


def test_negative_zero_gradient_on_a_negative_zero_row(dr, orc):
    """0.0f + g decides the sign: a lone -0.0 gradient is summed to +0.0."""
    for D in (1, 4):
        w = np.full((3, D), -0.0, np.float32)
        g = np.full((1, D), -0.0, np.float32)
        idx = np.array([1], np.int64)
        tab = Tab(w, SGD)
        c_apply(dr, SGD, [(tab, T(g), T(idx), None)])
        ref.apply_sgd(orc, w, LR, idx, g)
        dr.status_check()
        assert same(tab.w, w)
        assert np.signbit(tab.w.cpu().numpy()).all()      # -0.0 - (+0.0) = -0.0


# ---------------------------------------------------------------------------
# 3. the device count
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [SGD, ADAGRAD, ADAM_ASYNC])
@pytest.mark.parametrize("count", [0, 1, 37, 64])
def test_device_count(dr, orc, opt, count):
    rng = np.random.default_rng(31)
    R, D, cap = 9, 4, 64
    idx = rng.integers(0, R, cap).astype(np.int64)
    g = rng.standard_normal((cap, D)).astype(np.float32)
    # past the count: indices far out of range and NaN values
    idx_d, g_d = idx.copy(), g.copy()
    idx_d[count:] = np.int64(1) << 40
    g_d[count:] = np.nan
    w = rng.standard_normal((R, D)).astype(np.float32)
    acc = np.full((R, D), 0.1, np.float32)
    tab = Tab(w, opt)
    before = tab.state()
    c_apply(dr, opt, [(tab, T(g_d), T(idx_d), T([count], torch.int64))])
    dr.status_check()                 # nothing past the count was looked at
    if count == 0:
        assert all(same(a, b) for a, b in zip(tab.state(), before))
        return
    if opt == ADAM_ASYNC:             # the values are test 6's; here: rows touched, powers once
        touched = np.zeros(R, bool)
        touched[idx[:count]] = True
        moved = (bits(tab.w) != bits(w)).any(1)
        assert np.array_equal(moved, touched)
        assert not torch.isnan(tab.w).any() and not torch.isnan(tab.s1).any()
        f = np.float32
        assert same(tab.pw, np.array([f(0.9) * f(0.9), f(0.999) * f(0.999)], f))
        return
    ref_apply(orc, opt, w, acc, idx[:count], g[:count])
    assert same(tab.w, w)
    if opt == ADAGRAD:
        assert same(tab.s1, acc)


# ---------------------------------------------------------------------------
# 4. an index >= rows inside the count
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [SGD, ADAGRAD])
def test_out_of_range_index_is_skipped_and_latches(dr, orc, opt):
    from deeprec_amd._lib import InvalidArgumentError
    rng = np.random.default_rng(41)
    R, D, n = 6, 4, 20
    idx = rng.integers(0, R, n).astype(np.int64)
    idx[7] = R
    g = rng.standard_normal((n, D)).astype(np.float32)
    w = rng.standard_normal((R, D)).astype(np.float32)
    acc = np.full((R, D), 0.1, np.float32)
    tab = Tab(w, opt)
    dr.status_check()
    c_apply(dr, opt, [(tab, T(g), T(idx), None)])
    with pytest.raises(InvalidArgumentError):
        dr.status_check()
    dr.status_check()                 # raised once, clear afterwards
    keep = np.arange(n) != 7
    ref_apply(orc, opt, w, acc, idx[keep], g[keep])
    assert same(tab.w, w)
    if opt == ADAGRAD:
        assert same(tab.s1, acc)


# ---------------------------------------------------------------------------
# 5. more tables than a launch group, mixed widths
# ---------------------------------------------------------------------------
def test_33_tables_of_mixed_shape_in_one_call(dr, orc):
    rng = np.random.default_rng(51)
    items, wants = [], []
    for t in range(33):
        D = (4, 6, 16)[t % 3]
        R = 5 + (t * 75) // 32
        n = 0 if t == 13 else int(rng.integers(1, 70))
        idx = rng.integers(-1, R, n).astype(np.int64)
        g = rng.standard_normal((n, D)).astype(np.float32)
        w = rng.standard_normal((R, D)).astype(np.float32)
        acc = np.full((R, D), 0.1, np.float32)
        tab = Tab(w, ADAGRAD)
        items.append((tab, T(g), T(idx), None))
        ref.apply_adagrad(orc, w, acc, LR, idx, g)
        wants.append((w, acc))
    assert sorted({it[0].w.shape[0] for it in items})[::32] == [5, 80]
    c_apply(dr, ADAGRAD, items)
    dr.status_check()
    for t, ((tab, _, _, _), (w, acc)) in enumerate(zip(items, wants)):
        assert same(tab.w, w) and same(tab.s1, acc), t


def test_33_tables_of_one_shape_are_cut_at_the_group_size(dr, orc):
    rng = np.random.default_rng(52)
    items, wants = [], []
    for t in range(33):
        R, D, n = 9 + t % 4, 6, 40
        idx = rng.integers(0, R, n).astype(np.int64)
        g = rng.standard_normal((n, D)).astype(np.float32)
        w = rng.standard_normal((R, D)).astype(np.float32)
        tab = Tab(w, SGD)
        items.append((tab, T(g), T(idx), None))
        ref.apply_sgd(orc, w, LR, idx, g)
        wants.append(w)
    c_apply(dr, SGD, items)
    dr.status_check()
    for t, ((tab, _, _, _), w) in enumerate(zip(items, wants)):
        assert same(tab.w, w), t


# every row shape of the kernel: 4-wide G = 1 .. 64 and 2 / 4 chunks per lane,
# scalar G = 4 .. 64 and 4 chunks per lane; widths below a shape's full width
# leave lanes idle (12, 30, 50, 200, 260, 520)
ALL_SHAPE_DIMS = [4, 8, 16, 32, 64, 128, 256, 260, 520, 1024, 3, 6, 12, 30, 50, 200, 256]


@pytest.mark.parametrize("opt", [SGD, ADAGRAD, ADAM_ASYNC, RMSPROP])
def test_tables_of_every_row_shape_in_one_call(dr, orc, opt):
    """One call over tables of every width class, 4-wide and scalar mixed in
    any order: each table runs its own shape.  The last table is 256 wide with
    a gradient block that is only 4-byte aligned (the scalar layout at a
    4-wide width).  SGD / Adagrad against the oracle; AdamAsync / RMSprop
    against the same tables applied one call each (the single-table result,
    pinned to the EV kernels by test_adam_async_equals_the_ev)."""
    rng = np.random.default_rng(53)
    order = rng.permutation(len(ALL_SHAPE_DIMS))
    items, alone, wants = [], [], []
    for j in order:
        D = ALL_SHAPE_DIMS[j]
        R, n = 6, 37
        idx = rng.integers(-1, R, n).astype(np.int64)
        g = rng.standard_normal((n, D)).astype(np.float32)
        w = rng.standard_normal((R, D)).astype(np.float32)
        acc = np.full((R, D), 0.1, np.float32)
        if j == len(ALL_SHAPE_DIMS) - 1:
            flat = torch.zeros(n * D + 1, dtype=torch.float32, device=DEV)
            gd = flat[1:].view(n, D)
            gd.copy_(T(g))
            assert gd.data_ptr() % 16 == 4
        else:
            gd = T(g)
        items.append((Tab(w, opt), gd, T(idx), None))
        alone.append((Tab(w, opt), gd, T(idx), None))
        if opt in (SGD, ADAGRAD):
            ref_apply(orc, opt, w, acc, idx, g)
        wants.append((w, acc))
    c_apply(dr, opt, items)
    for it in alone:
        c_apply(dr, opt, [it])
    dr.status_check()
    for (tab, _, _, _), (one, _, _, _), (w, acc), j in zip(items, alone, wants, order):
        D = ALL_SHAPE_DIMS[j]
        assert all(same(a, b) for a, b in zip(tab.state(), one.state())), D
        if opt in (SGD, ADAGRAD):
            assert same(tab.w, w), D
        if opt == ADAGRAD:
            assert same(tab.s1, acc), D
        if opt in (ADAM_ASYNC, RMSPROP):          # (w is still the initial table here)
            assert not same(tab.w, w), D


# ---------------------------------------------------------------------------
# 6. AdamAsync / RMSprop: a dense table steps exactly as an EV with its rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rmsprop", [False, True])
@pytest.mark.parametrize("D", [4, 6])
def test_adam_async_equals_the_ev(dr, D, rmsprop):
    rng = np.random.default_rng(61 + D)
    R, n = 11, 90
    keys = np.arange(R, dtype=np.int64)
    w0 = rng.standard_normal((R, D)).astype(np.float32)
    _N[0] += 1
    ev = dr.EmbeddingVariable("da_ev%d" % _N[0], D, 0.0)
    ev.insert(T(keys), T(w0))
    tab = dr.DenseTable(T(w0.copy()))
    o_ev = dr.AdamAsyncOptimizer(0.01, apply_sparse_rmsprop=rmsprop)
    o_tab = dr.AdamAsyncOptimizer(0.01, apply_sparse_rmsprop=rmsprop)
    f = np.float32
    b1p, b2p = f(0.9), f(0.999)
    for step in range(4):
        idx = rng.integers(0, R - 2, n).astype(np.int64)       # repeats; rows R-2, R-1 untouched
        g = (rng.standard_normal((n, D)) * 0.3).astype(np.float32)
        if step == 2:                 # an empty step (device count 0): nothing moves
            u = np.arange(4, dtype=np.int64)
            for var in (ev, tab):
                var.pending_grads.append(dr.IndexedSlices(T(g[:4]), T(u), T([0], torch.int64),
                                                          unique=True))
        else:
            for var in (ev, tab):
                var.pending_grads.append(dr.IndexedSlices(T(g), T(idx)))
            b1p, b2p = b1p * f(0.9), b2p * f(0.999)
        o_ev.apply_gradients([ev], global_step=step)
        o_tab.apply_gradients([tab], global_step=step)
        dr.status_check()
        m, v = o_tab._dense_mv[id(tab)]
        assert same(tab.weight, ev.sparse_read(T(keys))), step
        assert same(m, ev.slot("AdamAsync", 0.0).sparse_read(T(keys))), step
        assert same(v, ev.slot("AdamAsync_1", 0.0).sparse_read(T(keys))), step
        if not rmsprop:
            assert o_tab._power(tab) == o_ev._power(ev) == [float(b1p), float(b2p)], step
    assert same(tab.weight[R - 2:], w0[R - 2:]) and not same(tab.weight, w0)


# ---------------------------------------------------------------------------
# 7. through the public surface
# ---------------------------------------------------------------------------
B, Q, R_ = 64, 7, 5
LENS = [0, 1, 2, 7, 8, 9, 10, 16, 17, 33]


def bags(seed, weighted):
    rng = np.random.default_rng(seed)
    lens = np.array(LENS + list(rng.choice(LENS, B - len(LENS))))
    rng.shuffle(lens)
    rows = np.repeat(np.arange(B), lens)
    cols = np.concatenate([np.arange(n) for n in lens])
    ind = np.stack([rows, cols], 1).astype(np.int64)
    ids = rng.integers(0, Q * Q, rows.size).astype(np.int64)
    w = rng.uniform(0.25, 2.0, rows.size).astype(np.float32) if weighted else None
    return ind, ids, w


@pytest.mark.parametrize("opt_name", ["sgd", "adagrad"])
@pytest.mark.parametrize("op", ["add", "mul"])
def test_five_multihash_training_steps_equal_the_cpu_reference(dr, orc, op, opt_name):
    D = 16
    rng = np.random.default_rng(80)
    tq = rng.standard_normal((Q, D)).astype(np.float32)
    tr = rng.standard_normal((R_, D)).astype(np.float32)
    aq, ar = np.full_like(tq, 0.1), np.full_like(tr, 0.1)
    _N[0] += 1
    v = dr.get_multihash_variable("da_mhv%d" % _N[0], [[Q, D], [R_, D]], operation=op,
                                  initializer=[T(tq), T(tr)], device=DEV)
    opt = dr.GradientDescentOptimizer(LR) if opt_name == "sgd" else \
        dr.AdagradOptimizer(LR, initial_accumulator_value=0.1)
    code = SGD if opt_name == "sgd" else ADAGRAD
    for step in range(5):
        ind, ids, w = bags(90 + step, step % 2 == 1)
        g = rng.standard_normal((B, D)).astype(np.float32)
        width = int(ind[:, 1].max()) + 1
        sp = dr.SparseTensor(T(ind), T(ids), (B, width))
        spw = None if w is None else dr.SparseTensor(T(ind), T(w), (B, width))
        res = dr.embedding_lookup_sparse(v, sp, spw, combiner="mean")
        res.backward(T(g))
        _, _, qi, qv, ri, rv = ref.lookup_sparse_grad(orc, tq, tr, op, ind, ids, B, g, weights=w)
        assert np.unique(qi).size < qi.size and np.unique(ri).size < ri.size      # repeats
        opt.apply_gradients([v], global_step=step)
        dr.status_check()
        ref_apply(orc, code, tq, aq, qi, qv)
        ref_apply(orc, code, tr, ar, ri, rv)
        assert same(v.val_list[0].weight, tq) and same(v.val_list[1].weight, tr), (op, step)
        if code == ADAGRAD:
            assert same(opt._dense_acc[id(v.val_list[0])], aq), step
            assert same(opt._dense_acc[id(v.val_list[1])], ar), step


@pytest.mark.parametrize("opt_name", ["sgd", "adagrad"])
def test_two_pending_slices_one_with_a_device_count(dr, orc, opt_name):
    rng = np.random.default_rng(71)
    R, D = 12, 6
    w = rng.standard_normal((R, D)).astype(np.float32)
    acc = np.full((R, D), 0.1, np.float32)
    tab = dr.DenseTable(T(w.copy()))
    opt = dr.GradientDescentOptimizer(LR) if opt_name == "sgd" else \
        dr.AdagradOptimizer(LR, initial_accumulator_value=0.1)
    code = SGD if opt_name == "sgd" else ADAGRAD
    for step, count in enumerate((9, 0, 20)):
        i1 = rng.integers(0, R, 30).astype(np.int64)
        g1 = rng.standard_normal((30, D)).astype(np.float32)
        i2 = rng.integers(0, R, 20).astype(np.int64)
        g2 = rng.standard_normal((20, D)).astype(np.float32)
        i2d, g2d = i2.copy(), g2.copy()
        i2d[count:] = np.int64(1) << 40           # garbage past the count
        g2d[count:] = np.nan
        tab.pending_grads.append(dr.IndexedSlices(T(g1), T(i1)))
        tab.pending_grads.append(dr.IndexedSlices(T(g2d), T(i2d), T([count], torch.int64)))
        opt.apply_gradients([tab], global_step=step)
        dr.status_check()
        ref_apply(orc, code, w, acc, np.concatenate([i1, i2[:count]]),
                  np.concatenate([g1, g2[:count]]))
        assert same(tab.weight, w), step
        if code == ADAGRAD:
            assert same(opt._dense_acc[id(tab)], acc), step


@pytest.mark.parametrize("opt_name", ["sgd", "adagrad"])
def test_a_wide_and_a_narrow_table_in_one_apply_gradients(dr, orc, opt_name):
    """[R, 512] (4-wide only: wider than the scalar layout reaches) next to
    [R, 6] (scalar only) on one device, in both orders."""
    rng = np.random.default_rng(72)
    opt = dr.GradientDescentOptimizer(LR) if opt_name == "sgd" else \
        dr.AdagradOptimizer(LR, initial_accumulator_value=0.1)
    code = SGD if opt_name == "sgd" else ADAGRAD
    ws = [rng.standard_normal((8, D)).astype(np.float32) for D in (512, 6)]
    accs = [np.full_like(w, 0.1) for w in ws]
    tabs = [dr.DenseTable(T(w.copy())) for w in ws]
    for step in range(2):
        for tab, w, acc in zip(tabs, ws, accs):
            idx = rng.integers(0, 8, 25).astype(np.int64)
            g = rng.standard_normal((25, w.shape[1])).astype(np.float32)
            tab.pending_grads.append(dr.IndexedSlices(T(g), T(idx)))
            ref_apply(orc, code, w, acc, idx, g)
        opt.apply_gradients(tabs[::-1] if step else tabs, global_step=step)
        dr.status_check()
        for tab, w, acc in zip(tabs, ws, accs):
            assert not tab.pending_grads
            assert same(tab.weight, w), (step, w.shape)
            if code == ADAGRAD:
                assert same(opt._dense_acc[id(tab)], acc), (step, w.shape)


# ---------------------------------------------------------------------------
# 8. under stream capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["sgd", "adagrad"])
def test_captured_apply_replays_with_new_slices(dr, orc, opt_name):
    rng = np.random.default_rng(91)
    R, D, cap = 10, 16, 48
    w = rng.standard_normal((R, D)).astype(np.float32)
    acc = np.full((R, D), 0.1, np.float32)
    tab = dr.DenseTable(T(w.copy()))
    opt = dr.GradientDescentOptimizer(LR) if opt_name == "sgd" else \
        dr.AdagradOptimizer(LR, initial_accumulator_value=0.1)
    code = SGD if opt_name == "sgd" else ADAGRAD
    vals = torch.zeros((cap, D), dtype=torch.float32, device=DEV)
    idxs = torch.zeros(cap, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)

    def fill(count):
        i = rng.integers(0, R, cap).astype(np.int64)
        g = rng.standard_normal((cap, D)).astype(np.float32)
        vals.copy_(T(g))
        idxs.copy_(T(i))
        cnt.fill_(count)
        return i[:count], g[:count]

    # one eager step first: the slots exist before the capture
    i, g = fill(cap)
    tab.pending_grads.append(dr.IndexedSlices(vals, idxs, cnt))
    opt.apply_gradients([tab], global_step=0)
    ref_apply(orc, code, w, acc, i, g)
    dr.status_check()
    assert same(tab.weight, w)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    tab.pending_grads.append(dr.IndexedSlices(vals, idxs, cnt))
    cnt.fill_(0)                      # the capture itself applies nothing
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        opt.apply_gradients([tab], global_step=1)
    for count in (31, 0, cap):
        i, g = fill(count)
        graph.replay()
        torch.cuda.synchronize()
        ref_apply(orc, code, w, acc, i, g)
        dr.status_check()
        assert same(tab.weight, w), count
        if code == ADAGRAD:
            assert same(opt._dense_acc[id(tab)], acc), count
