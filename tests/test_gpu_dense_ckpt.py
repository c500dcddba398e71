"""Checkpoints of dense tables, composite variables and optimizer state on the
GPU.  Every comparison is bit equality (NaNs must coincide).

1. The C entries of csrc/dense_ckpt.hip (mark, mark all, clear, count, export,
   upsert) against the numpy model tests/dense_ckpt_ref.py: rows 1, 31, 32, 33,
   64, 1000 (both sides of a word boundary, several blocks of words), row
   widths 1, 4, 6, 16, 128, 200, 520 (scalar and 4-wide shapes, one and several
   chunks per lane), and 2 097 185 rows at width 1 -- 65 538 words, the first
   size past the scan's one-block path.
2. Marking under stream capture.
3. Tracking through apply_gradients for every optimizer, against an untracked
   twin.
4. Resume: three steps, a full save with optimizer.checkpoint_variables, fresh
   variables and a fresh optimizer, restore, two more steps -- equal to the
   uninterrupted five-step twin.  B = 64, ids in [0, 49); the EV and the
   adaptive feature also see -7 and 2^40 + 3 (a dense table and a multi-hash
   variable take row ids, for which those are errors).
5. Deltas: a tracked trainer feeds a replica a full save and three deltas."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_ckpt_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = [1, 31, 32, 33, 64, 1000]
DIMS = [1, 4, 6, 16, 128, 200, 520]
BIG_ROWS = 2097185
HUGE = 1 << 40
_N = [0]


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    from deeprec_amd._lib import DrDenseMarkDesc  # noqa: F401  (the feature under test)
    deeprec_amd.load()
    deeprec_amd.set_validate(True)
    assert torch.cuda.is_available()
    return deeprec_amd


def T(x, dtype=None):
    return torch.as_tensor(np.asarray(x), device=DEV, dtype=dtype)


def N(t):
    return t.detach().cpu().numpy()


def same(a, b):
    """Bit equality of two arrays, NaNs at the same places."""
    a = N(a) if torch.is_tensor(a) else np.asarray(a)
    b = N(b) if torch.is_tensor(b) else np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def L():
    from deeprec_amd import _lib
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits_t(bits):
    """uint32 numpy words -> the int32 device tensor that holds them."""
    return T(np.asarray(bits, np.uint32).view(np.int32).copy())


def bits_np(t):
    return N(t).view(np.uint32)


# ---------------------------------------------------------------------------
# the C entries on torch tensors
# ---------------------------------------------------------------------------
def c_mark(items):
    """items: (bits tensor or None, rows, idx tensor, device count or None)."""
    lib = L()
    descs = (lib.DrDenseMarkDesc * len(items))()
    for d, (b, rows, idx, n_dev) in zip(descs, items):
        d.bits = None if b is None else b.data_ptr()
        d.rows, d.idx, d.n = rows, idx.data_ptr() if idx.numel() else None, idx.numel()
        d.n_dev = None if n_dev is None else n_dev.data_ptr()
    lib.check(lib.lib().dr_dense_mark_rows(descs, len(items), stream()))


def c_count(bits, rows):
    lib = L()
    out = T([-1], torch.int64)
    lib.check(lib.lib().dr_dense_marked_count(bits.data_ptr(), rows, out.data_ptr(), stream()))
    return int(out.item())


PAD = 3             # guard rows behind every output block


def c_export(bits, rows, dim, cols, capacity):
    """(m, rows_out [capacity + PAD], [vals [capacity + PAD, dim]]): the
    outputs start as sentinels, the guard rows must come back untouched."""
    lib = L()
    rows_out = torch.full((capacity + PAD,), -77, dtype=torch.int64, device=DEV)
    vals = [torch.full((capacity + PAD, dim), -77.0, device=DEV) for _ in cols]
    m_dev = T([-1], torch.int64)
    P = C.c_void_p * max(len(cols), 1)
    wsb = lib.lib().dr_dense_export_marked_workspace_size(rows)
    ws = lib.workspace(wsb, DEV)
    lib.check(lib.lib().dr_dense_export_marked(
        bits.data_ptr(), rows, dim, P(*[c.data_ptr() for c in cols]), len(cols), capacity,
        rows_out.data_ptr(), P(*[v.data_ptr() for v in vals]), m_dev.data_ptr(), ws.data_ptr(),
        wsb, stream()))
    return int(m_dev.item()), N(rows_out), [N(v) for v in vals]


def c_upsert(cols, rows, dim, idx, vals, n_dev=None):
    lib = L()
    P = C.c_void_p * len(cols)
    lib.check(lib.lib().dr_dense_upsert_rows(
        P(*[c.data_ptr() for c in cols]), len(cols), rows, dim, idx.data_ptr(), idx.numel(),
        None if n_dev is None else n_dev.data_ptr(), P(*[v.data_ptr() for v in vals]), stream()))


def index_sets(rows, rng):
    rep = rng.integers(0, rows, 50).astype(np.int64)
    mixed = rng.integers(0, rows, 41).astype(np.int64)
    mixed[::5] = -1
    mixed[2::7] = rows
    mixed[3::11] = rows + 31
    mixed[4::13] = HUGE
    return {
        "empty": np.zeros(0, np.int64),
        "every": np.arange(rows, dtype=np.int64),
        "every32": np.arange(0, rows, 32, dtype=np.int64),
        "last": np.array([rows - 1], np.int64),
        "repeated": np.concatenate([rep, rep[::-1], rep[:7]]),
        "mixed": mixed,
    }


def check_export(bits_dev, bits_host, rows, dim, cols_dev, cols_host, capacity):
    m, rows_out, vals = c_export(bits_dev, rows, dim, cols_dev, capacity)
    wm, wrows, wvals = ref.export(bits_host, rows, cols_host, capacity)
    k = min(wm, capacity)
    assert m == wm, (rows, dim, capacity)
    assert np.array_equal(rows_out[:k], wrows), (rows, dim, capacity)
    assert (rows_out[k:] == -77).all(), "a row id was written at or past the capacity / count"
    for v, wv in zip(vals, wvals):
        assert same(v[:k], wv), (rows, dim, capacity)
        assert (v[k:] == -77.0).all(), "a value row was written at or past the capacity / count"
    return m


# ---------------------------------------------------------------------------
# 1. the C entries against the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
def test_mark_and_count(dr, rows):
    rng = np.random.default_rng(100 + rows)
    for name, idx in index_sets(rows, rng).items():
        # what lies past the count: ids that would be far outside the table
        buf = np.concatenate([idx, np.full(3, HUGE, np.int64)])
        for count in (None, 0, 1, 37, idx.size, buf.size):
            host = ref.mark(ref.new_bits(rows), rows, [5 % rows])       # a mark that stays
            dev = bits_t(host)
            n_dev = None if count is None else T([count], torch.int64)
            c_mark([(dev, rows, T(buf), n_dev)])
            host = ref.mark(host, rows, buf, count)
            assert np.array_equal(bits_np(dev), host), (rows, name, count)
            assert c_count(dev, rows) == ref.count(host, rows), (rows, name, count)
        if idx.size == 0:                                  # n == 0: nothing is launched
            dev = bits_t(ref.new_bits(rows))
            c_mark([(dev, rows, T(idx), None)])
            assert c_count(dev, rows) == 0
    dr.status_check()               # an index out of range latches nothing here


@pytest.mark.parametrize("rows", ROWS)
def test_mark_all_clear_and_tail_bits(dr, rows):
    lib = L()
    nw = ref.words(rows)
    dev = bits_t(np.full(nw, 0xA5A5A5A5, np.uint32))
    lib.check(lib.lib().dr_dense_mark_all(dev.data_ptr(), rows, stream()))
    assert np.array_equal(bits_np(dev), ref.mark_all(rows))         # the tail written as 0
    assert c_count(dev, rows) == rows
    lib.check(lib.lib().dr_dense_clear_marks(dev.data_ptr(), rows, stream()))
    assert not bits_np(dev).any() and c_count(dev, rows) == 0
    # hand-set tail bits of the last word are ignored by count and export
    host = ref.mark(ref.new_bits(rows), rows, [0, rows - 1])
    if rows % 32:
        host[-1] |= np.uint32(0xFFFFFFFF & ~ref.tail_mask(rows))
    dev = bits_t(host)
    assert c_count(dev, rows) == len({0, rows - 1})
    w = np.arange(rows * 4, dtype=np.float32).reshape(rows, 4)
    check_export(dev, host, rows, 4, [T(w)], [w], rows)
    dr.status_check()


def test_mark_33_tables_in_one_call(dr):
    rng = np.random.default_rng(7)
    sizes = [1 + (37 * t) % 90 for t in range(33)]
    hosts = [ref.new_bits(r) for r in sizes]
    devs = [bits_t(h) for h in hosts]
    items, keep = [], []
    for t, r in enumerate(sizes):
        idx = rng.integers(-2, r + 2, 1 + (11 * t) % 40).astype(np.int64)
        count = None if t % 3 else int(rng.integers(0, idx.size + 1))
        keep.append((idx, count))
        items.append((devs[t], r, T(idx), None if count is None else T([count], torch.int64)))
        hosts[t] = ref.mark(hosts[t], r, idx, count)
    # two more descriptors: the first table's marks again, and one without marks (skipped)
    extra = np.array([0, sizes[0] - 1], np.int64)
    items.insert(5, (devs[0], sizes[0], T(extra), None))
    hosts[0] = ref.mark(hosts[0], sizes[0], extra)
    items.insert(20, (None, 10, T(np.array([HUGE], np.int64)), None))
    assert len(items) == 35 and len({id(i[0]) for i in items if i[0] is not None}) == 33
    c_mark(items)
    for t in range(33):
        assert np.array_equal(bits_np(devs[t]), hosts[t]), t
    dr.status_check()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_export(dr, rows, dim):
    rng = np.random.default_rng(rows * 1000 + dim)
    cols = [rng.standard_normal((rows, dim)).astype(np.float32) for _ in range(3)]
    cols[0][0, 0], cols[1][rows - 1, dim - 1] = np.nan, -0.0
    cols_dev = [T(c) for c in cols]
    sets = index_sets(rows, rng)
    for name in ("every", "every32", "last", "repeated", "empty"):
        host = ref.mark(ref.new_bits(rows), rows, sets[name])
        dev = bits_t(host)
        m = ref.count(host, rows)
        for ncols in (1, 2, 3):
            got = check_export(dev, host, rows, dim, cols_dev[:ncols], cols[:ncols], m)
            assert got == m
        if m > 1:           # a capacity below m: the overflow is reported, not written
            check_export(dev, host, rows, dim, cols_dev[:2], cols[:2], m - 1)
            check_export(dev, host, rows, dim, cols_dev[:1], cols[:1], 1)
        check_export(dev, host, rows, dim, cols_dev[:1], cols[:1], m + 5)
        check_export(dev, host, rows, dim, [], [], m)               # the row ids alone
        check_export(dev, host, rows, dim, cols_dev[:1], cols[:1], 0)
    for c, d in zip(cols, cols_dev):
        assert same(d, c)                                           # the export only reads
    dr.status_check()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_upsert(dr, rows, dim):
    rng = np.random.default_rng(rows * 77 + dim)
    n = min(rows, 45)
    idx = rng.permutation(rows)[:n].astype(np.int64)
    for ncols in (1, 2):
        for count in (None, 0, 1, 37, n):
            if count is None or count > n:
                i_host, k = idx, n          # no device count, or one above the capacity
            else:
                # past the count: ids far outside the table and NaN rows
                i_host, k = np.concatenate([idx[:count], np.full(2, HUGE, np.int64)]), count
            cols = [rng.standard_normal((rows, dim)).astype(np.float32) for _ in range(ncols)]
            vals = [np.concatenate([rng.standard_normal((k, dim)).astype(np.float32),
                                    np.full((i_host.size - k, dim), np.nan, np.float32)])
                    for _ in range(ncols)]
            if k:
                vals[0][0, 0] = -0.0
            cols_dev = [T(c) for c in cols]
            c_upsert(cols_dev, rows, dim, T(i_host), [T(v) for v in vals],
                     None if count is None else T([count], torch.int64))
            want, latched = ref.upsert(cols, rows, i_host, vals, count)
            assert not latched
            for d, w in zip(cols_dev, want):
                assert same(d, w), (rows, dim, ncols, count)
    dr.status_check()               # nothing past the count was looked at


def test_upsert_out_of_range_is_skipped_and_latches(dr):
    from deeprec_amd._lib import InvalidArgumentError
    rng = np.random.default_rng(5)
    rows, dim = 33, 6
    for bad in (-1, rows, HUGE):
        idx = np.array([4, bad, 32, 0], np.int64)
        cols = [rng.standard_normal((rows, dim)).astype(np.float32) for _ in range(2)]
        vals = [rng.standard_normal((4, dim)).astype(np.float32) for _ in range(2)]
        cols_dev = [T(c) for c in cols]
        dr.status_check()
        c_upsert(cols_dev, rows, dim, T(idx), [T(v) for v in vals])
        with pytest.raises(InvalidArgumentError):
            dr.status_check()
        dr.status_check()               # raised once, clear afterwards
        want, latched = ref.upsert(cols, rows, idx, vals)
        assert latched
        for d, w in zip(cols_dev, want):
            assert same(d, w), bad


def test_big_table_takes_the_tiled_scan(dr):
    """65 538 words: one past the scan's one-block limit of 65 536."""
    rows = BIG_ROWS
    assert ref.words(rows) == 65538
    lib = L()
    rng = np.random.default_rng(11)
    idx = np.concatenate([np.arange(0, rows, 32, dtype=np.int64), [rows - 1, rows - 2, 0],
                          rng.integers(0, rows, 5000).astype(np.int64), [-1, rows, HUGE]])
    host = ref.mark(ref.new_bits(rows), rows, idx)
    dev = bits_t(ref.new_bits(rows))
    c_mark([(dev, rows, T(idx), None)])
    assert np.array_equal(bits_np(dev), host)
    m = ref.count(host, rows)
    assert m > 65538 and c_count(dev, rows) == m
    w = rng.standard_normal((rows, 1)).astype(np.float32)
    w_dev = T(w)
    assert check_export(dev, host, rows, 1, [w_dev], [w], m) == m
    check_export(dev, host, rows, 1, [w_dev], [w], 1000)            # an overflow on this path
    lib.check(lib.lib().dr_dense_mark_all(dev.data_ptr(), rows, stream()))
    assert c_count(dev, rows) == rows
    assert np.array_equal(bits_np(dev), ref.mark_all(rows))
    dr.status_check()


# ---------------------------------------------------------------------------
# the DenseTable surface
# ---------------------------------------------------------------------------
def test_dense_table_methods(dr):
    rng = np.random.default_rng(21)
    rows, dim = 70, 6
    w = rng.standard_normal((rows, dim)).astype(np.float32)
    t = dr.DenseTable(T(w.copy()), name="bucket")
    assert t.name == "bucket" and not t.tracking_updates()
    t.mark_updated(T(np.array([1, 2], np.int64)))           # a no-op while tracking is off
    with pytest.raises(dr.InvalidArgumentError, match="bucket.*not tracking"):
        t.export_updated()
    t.track_updates()
    assert t.tracking_updates() and t.updated_count() == 0
    idx = np.array([69, 3, 3, 64, -1, 70, HUGE], np.int64)
    t.mark_updated(T(idx))
    t.mark_updated(T(np.array([5, 6, 7], np.int64)), T([1], torch.int64))
    t.track_updates()                                        # on while on keeps the marks
    r, v = t.export_updated()
    assert r.dtype == torch.int64 and N(r).tolist() == [3, 5, 64, 69]
    assert same(v, w[[3, 5, 64, 69]]) and t.updated_count() == 4
    t.clear_updated()
    assert t.updated_count() == 0 and t.export_updated()[0].numel() == 0
    new = rng.standard_normal((2, dim)).astype(np.float32)
    t.upsert(T(np.array([69, 0], np.int64)), T(new))
    w[[69, 0]] = new
    assert same(t.weight, w)
    t.track_updates(False)
    assert not t.tracking_updates()
    wide = dr.DenseTable(torch.zeros((4, 258), device=DEV), name="wide")
    with pytest.raises(dr.InvalidArgumentError, match="wide.*258"):
        wide.track_updates()
    dr.status_check()


# ---------------------------------------------------------------------------
# 2. marking under capture
# ---------------------------------------------------------------------------
def test_captured_mark_and_apply_follow_the_replayed_indices(dr):
    rng = np.random.default_rng(91)
    R, D, cap = 70, 16, 48
    w = rng.standard_normal((R, D)).astype(np.float32)
    tab, twin = dr.DenseTable(T(w.copy())), dr.DenseTable(T(w.copy()))
    tab.track_updates()
    opt, opt2 = dr.AdagradOptimizer(0.05), dr.AdagradOptimizer(0.05)
    vals = torch.zeros((cap, D), dtype=torch.float32, device=DEV)
    idxs = torch.zeros(cap, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)

    def fill(count):
        i = rng.integers(0, R, cap).astype(np.int64)
        i[count:] = HUGE                   # what lies past the count is never a row id
        vals.copy_(T(rng.standard_normal((cap, D)).astype(np.float32)))
        idxs.copy_(T(i))
        cnt.fill_(count)
        return i[:count]

    def twin_step(step):
        twin.pending_grads.append(dr.IndexedSlices(vals.clone(), idxs.clone(), cnt.clone()))
        opt2.apply_gradients([twin], global_step=step)

    # one eager step first: the slots exist before the capture
    i = fill(cap)
    tab.pending_grads.append(dr.IndexedSlices(vals, idxs, cnt))
    opt.apply_gradients([tab], global_step=0)
    twin_step(0)
    host = ref.mark(ref.new_bits(R), R, i)
    assert np.array_equal(bits_np(tab._bits), host)
    tab.clear_updated()
    host = ref.new_bits(R)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    tab.pending_grads.append(dr.IndexedSlices(vals, idxs, cnt))
    cnt.fill_(0)                           # the capture itself applies and marks nothing
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        opt.apply_gradients([tab], global_step=1)
    assert not bits_np(tab._bits).any()
    for step, count in enumerate((5, 0, 31, cap)):
        i = fill(count)
        graph.replay()
        torch.cuda.synchronize()
        twin_step(1 + step)
        host = ref.mark(host, R, i)
        dr.status_check()
        assert np.array_equal(bits_np(tab._bits), host), count
        assert same(tab.weight, twin.weight), count
    assert same(opt._dense_acc[id(tab)], opt2._dense_acc[id(twin)])
    assert 0 < ref.count(host, R) < R


# ---------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------
OPTS = ["sgd", "adagrad", "adam", "ftrl", "adam_async", "adam_async_rmsprop", "adagrad_decay"]


def make_opt(dr, name):
    if name == "sgd":
        return dr.GradientDescentOptimizer(0.05)
    if name == "adagrad":
        return dr.AdagradOptimizer(0.05, initial_accumulator_value=0.1)
    if name == "adam":
        return dr.AdamOptimizer(0.01)
    if name == "ftrl":
        return dr.FtrlOptimizer(0.05, l1_regularization_strength=0.001,
                                l2_regularization_strength=0.01)
    if name == "adam_async":
        return dr.AdamAsyncOptimizer(0.01)
    if name == "adam_async_rmsprop":
        return dr.AdamAsyncOptimizer(0.01, apply_sparse_rmsprop=True)
    assert name == "adagrad_decay"
    # a decay step of 2: the per-row decay count moves inside five steps
    return dr.AdagradDecayOptimizer(0.05, initial_accumulator_value=0.1,
                                    accumulator_decay_step=2, accumulator_decay_rate=0.9)


def state_arrays(state):
    """{tensor key: numpy} of a state dict: tables, dense slots and scalars
    whole, an EV (primary or slot) as its export sorted by key."""
    from deeprec_amd import checkpoint as ck
    out = {}
    for k, v in ck.expand_variables(state).items():
        if hasattr(v, "get"):
            out[k] = np.float32(v.get())
        elif hasattr(v, "weight"):
            out[k] = N(v.weight)
        else:
            keys, vals, vers, frqs = [N(x) for x in v.export()]
            order = np.argsort(keys, kind="stable")
            out[k + "#keys"], out[k + "#values"] = keys[order], vals[order]
            out[k + "#versions"] = vers[order] if vers.size else vers
            out[k + "#freqs"] = frqs[order] if frqs.size else frqs
    return out


def assert_same_state(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert same(a[k], b[k]), (what, k)


# ---------------------------------------------------------------------------
# 3. tracking through apply_gradients
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", OPTS)
def test_apply_gradients_marks_the_pending_rows(dr, opt_name):
    rng = np.random.default_rng(31)
    R, D = 70, 4
    w = rng.standard_normal((R, D)).astype(np.float32)
    tab, twin = dr.DenseTable(T(w.copy()), name="tracked"), dr.DenseTable(T(w.copy()))
    cold = dr.DenseTable(T(w.copy()))           # has gradients, does not track: nothing runs
    tab.track_updates()
    o1, o2 = make_opt(dr, opt_name), make_opt(dr, opt_name)
    host = ref.new_bits(R)
    for step in range(3):
        i1 = rng.integers(0, R // 2, 9).astype(np.int64)
        i1[::4] = -1                                        # a skipped index inside the count
        count = int(rng.integers(2, 9))
        i1d = np.concatenate([i1, np.full(3, HUGE, np.int64)])
        g1 = np.concatenate([rng.standard_normal((9, D)).astype(np.float32),
                             np.full((3, D), np.nan, np.float32)])
        i2 = rng.integers(R // 2, R, 6).astype(np.int64)
        i2[1] = i2[0]                                       # a repeat
        g2 = rng.standard_normal((6, D)).astype(np.float32)
        for t in (tab, twin, cold):
            t.pending_grads.append(dr.IndexedSlices(T(g1), T(i1d), T([count], torch.int64)))
            t.pending_grads.append(dr.IndexedSlices(T(g2), T(i2)))
        o1.apply_gradients([tab, cold], global_step=step)
        o2.apply_gradients([twin], global_step=step)
        dr.status_check()
        assert cold._bits is None and not tab.pending_grads
        host = ref.mark_all(R) if opt_name == "adam" else \
            ref.mark(ref.mark(host, R, i1d, count), R, i2)
        assert np.array_equal(bits_np(tab._bits), host), (opt_name, step)
        r, v = tab.export_updated()
        assert np.array_equal(N(r), ref.marked_rows(host, R)) and same(v, N(tab.weight)[N(r)])
        if step == 1:
            tab.clear_updated()
            host = ref.new_bits(R)
    assert opt_name == "adam" or 0 < ref.count(host, R) < R
    # a tracked table trains to the same bits as an untracked one, slots included
    assert_same_state(state_arrays(dict({"t": tab}, **o1.checkpoint_variables({"t": tab}))),
                      state_arrays(dict({"t": twin}, **o2.checkpoint_variables({"t": twin}))),
                      opt_name)
    assert not same(tab.weight, w)


# ---------------------------------------------------------------------------
# 4 / 5. a small model: an EV, a hash-bucket table, two multi-hash variables
# and an adaptive variable with a Counter filter
# ---------------------------------------------------------------------------
B, NIDS, Q, R_, BUCKET = 64, 49, 7, 5, 11
ODD_IDS = (-7, HUGE + 3)
LENS = [0, 1, 2, 3, 7, 9]


class Model(object):
    FEATURES = ("ev", "bucket", "mh_add", "mh_cat", "ad")

    def __init__(self, dr, D, track=False):
        _N[0] += 1
        n = _N[0]
        rng = np.random.default_rng(400 + D)        # the same start for every instance
        t = lambda *shape: T(rng.standard_normal(shape).astype(np.float32))
        self.dr, self.D = dr, D
        self.v = {
            "ev": dr.EmbeddingVariable("ck_ev%d" % n, D, 0.25),
            "bucket": dr.DenseTable(t(NIDS, D), name="ck_bucket%d" % n),
            "mh_add": dr.get_multihash_variable("ck_mha%d" % n, [[Q, D], [R_, D]],
                                                operation="add",
                                                initializer=[t(Q, D), t(R_, D)], device=DEV),
            "mh_cat": dr.get_multihash_variable("ck_mhc%d" % n, [[Q, D], [R_, D // 2]],
                                                operation="concat",
                                                initializer=[t(Q, D), t(R_, D // 2)], device=DEV),
            "ad": dr.get_adaptive_embedding_variable(
                "ck_ad%d" % n, D, BUCKET, initializer=t(BUCKET, D),
                ev_option=dr.EmbeddingVariableOption(
                    filter_option=dr.CounterFilter(filter_freq=3)), device=DEV),
        }
        if track:
            self.v["ev"].track_updates()
            self.v["ad"].ev.track_updates()
            for t_ in self.dense_tables().values():
                t_.track_updates()

    def dense_tables(self):
        from deeprec_amd import checkpoint as ck
        return {k: x for k, x in ck.expand_variables(self.v).items() if hasattr(x, "weight")}

    @staticmethod
    def batch(step, feature, negative_from=None):
        """(indices [nnz, 2], ids [nnz], mask [nnz]) of one feature at one step.
        The EV and the adaptive feature also see 2^40 + 3 and, from step
        `negative_from` on, -7: the bundle format keeps no negative key
        (DumpEmbeddingValues groups by the C++ remainder key % 1000), so a
        negative key can only equal the uninterrupted twin's when it is
        created after the save.  The adaptive feature's ids (odd ones live in
        its EV, behind a Counter filter of 3) each come at least three times
        in a step, so no key is between its first sight and its admission
        when a checkpoint is written: export() keeps no such key."""
        rng = np.random.default_rng(1000 * step + Model.FEATURES.index(feature))
        lens = rng.choice(LENS, B)
        rows = np.repeat(np.arange(B), lens)
        cols = np.concatenate([np.arange(k) for k in lens])
        ind = np.stack([rows, cols], 1).astype(np.int64)
        if feature == "ad":
            ids = ((np.arange(rows.size) * 5 + 3 * step) % NIDS).astype(np.int64)
            assert np.bincount(ids, minlength=NIDS).min() >= 3
        else:
            ids = rng.integers(0, NIDS, rows.size).astype(np.int64)
        if feature in ("ev", "ad"):
            odd = [ODD_IDS[1]] * 3
            if negative_from is not None and step >= negative_from:
                odd += [ODD_IDS[0]] * 3
            for x, k in zip(odd, rng.choice(rows.size, len(odd), replace=False)):
                ids[k] = x
            assert np.bincount(ids[(ids >= 0) & (ids < NIDS)], minlength=NIDS).min() >= \
                (3 if feature == "ad" else 0)
        return ind, ids, (ids & 1).astype(np.int64)

    def sp(self, ind, ids):
        return self.dr.SparseTensor(T(ind), T(ids), (B, int(ind[:, 1].max()) + 1))

    negative_from = None

    def lookup(self, step, feature):
        ind, ids, mask = self.batch(step, feature, self.negative_from)
        kw = {"adaptive_mask_tensor": T(mask)} if feature == "ad" else {}
        return self.dr.embedding_lookup_sparse(self.v[feature], self.sp(ind, ids),
                                               combiner="mean", **kw)

    def train(self, opt, step, before_apply=None):
        for f in self.FEATURES:
            out = self.lookup(step, f)
            g = np.random.default_rng(77 * step + len(f)).standard_normal(
                tuple(out.shape)).astype(np.float32)
            out.backward(T(g))
        if before_apply:
            before_apply()
        opt.apply_gradients([self.v[f] for f in self.FEATURES], global_step=step)
        self.dr.status_check()

    def state(self, opt):
        s = dict(self.v)
        s.update(opt.checkpoint_variables(self.v))
        return s


@pytest.mark.parametrize("D", [4, 16])
@pytest.mark.parametrize("opt_name", OPTS)
def test_resume_equals_the_uninterrupted_twin(dr, tmp_path, opt_name, D):
    from deeprec_amd import checkpoint as ck
    twin, o_twin = Model(dr, D), make_opt(dr, opt_name)
    twin.negative_from = 3
    for step in range(5):
        twin.train(o_twin, step)
    first, o1 = Model(dr, D), make_opt(dr, opt_name)
    for step in range(3):
        first.train(o1, step)
    prefix = ck.save(str(tmp_path / "model"), first.state(o1))
    keys = ck.BundleReader(prefix).keys()
    assert "bucket" in keys and "mh_add/Q" in keys and "mh_cat/R" in keys and "ad/hash" in keys
    assert "ad/ev-keys" in keys and "ev-values" in keys
    if opt_name != "sgd":
        slot = o1._slot_names[0]
        assert "bucket/" + slot in keys and "ad/hash/" + slot in keys
        assert "ev/%s-keys" % slot in keys and "ad/ev/%s-values" % slot in keys
    second, o2 = Model(dr, D), make_opt(dr, opt_name)
    second.negative_from = 3
    ck.restore(prefix, second.state(o2))
    assert_same_state(state_arrays(second.state(o2)), state_arrays(first.state(o1)),
                      (opt_name, "restored"))
    for step in range(3, 5):
        second.train(o2, step)
    got, want = state_arrays(second.state(o2)), state_arrays(twin.state(o_twin))
    assert_same_state(got, want, (opt_name, D))
    assert got["ev#keys"].size > 40 and set(ODD_IDS) <= set(got["ev#keys"].tolist())
    assert set(ODD_IDS) <= set(got["ad/ev#keys"].tolist())
    assert not same(got["bucket"], state_arrays(first.state(o1))["bucket"])   # it went on training
    if opt_name in ("adam", "adam_async"):
        # the powers went on from the restored values: beta1 * beta1^5 in fp32
        p = np.float32(0.9)
        for _ in range(5):
            p = np.float32(p * np.float32(0.9))
        for k in (["beta1_power"] if opt_name == "adam" else
                  ["%s/beta1_power" % t for t in ("ev", "bucket", "mh_cat/R", "ad/hash", "ad/ev")]):
            assert got[k] == p, k


@pytest.mark.parametrize("opt_name", ["adagrad", "adam", "adagrad_decay"])
def test_deltas_feed_a_replica(dr, tmp_path, opt_name):
    from deeprec_amd import checkpoint as ck
    D = 16
    trainer, o_t = Model(dr, D, track=True), make_opt(dr, opt_name)
    replica, o_r = Model(dr, D), make_opt(dr, opt_name)
    tables = trainer.dense_tables()
    touched = {}

    def note():
        """The valid rows the pending slices name, read before the apply."""
        for k, t in tables.items():
            for sl in t.pending_grads:
                n = sl.indices.numel() if sl.num_valid is None else int(sl.num_valid.item())
                i = N(sl.indices)[:n]
                rows = t.weight.shape[0]
                touched.setdefault(k, set()).update(i[(i >= 0) & (i < rows)].tolist())

    for step in range(2):
        trainer.train(o_t, step, note)
    full = ck.save(str(tmp_path / "full"), trainer.state(o_t))
    for t in tables.values():
        t.clear_updated()                   # the full save holds everything so far
    trainer.v["ev"].clear_updated()
    trainer.v["ad"].ev.clear_updated()
    ck.restore(full, replica.state(o_r))
    slots = o_t._slot_names
    for step in range(2, 5):
        touched.clear()
        trainer.train(o_t, step, note)
        delta = ck.save_incremental(str(tmp_path / ("delta%d" % step)), trainer.state(o_t))
        r = ck.BundleReader(delta)
        for k, t in tables.items():
            rows = t.weight.shape[0]
            want = np.arange(rows) if opt_name == "adam" else np.array(sorted(touched[k]))
            assert want.size > 0
            got = r.lookup(k + "-sparse_incr_keys")
            assert got.dtype == np.int64 and np.array_equal(got, want), (step, k)
            model = ref.delta_tensors(
                k, ref.mark(ref.new_bits(rows), rows, want), N(t.weight),
                [(s, N(o_t.checkpoint_variables({k: t})["%s/%s" % (k, s)].weight))
                 for s in slots])
            for name, a in model.items():
                assert same(r.lookup(name), a), (step, name)
            assert t.updated_count() == 0               # cleared once, after all its columns
        ck.restore_incremental(delta, replica.state(o_r))
        dr.status_check()
        assert_same_state(state_arrays(replica.state(o_r)), state_arrays(trainer.state(o_t)),
                          (opt_name, step))
    # read-only lookups on the replica serve what the trainer's do
    with dr.read_only_lookups():
        for m in (trainer, replica):
            outs = [m.lookup(9, f) for f in ("mh_add", "mh_cat", "ad")]
            ind, ids, mask = Model.batch(9, "ad")
            ind2, ids2, _ = Model.batch(9, "mh_add")
            multi = dr.embedding_lookup_sparse_multi(
                [m.v["mh_add"], m.v["ad"], m.v["bucket"]],
                [m.sp(ind2, ids2), m.sp(ind, ids), m.sp(ind2, ids2)], combiner="mean",
                adaptive_masks=[None, T(mask), None])
            m.served = [N(o) for o in outs] + [N(multi)]
    for a, b in zip(trainer.served, replica.served):
        assert same(a, b)
    assert same(trainer.served[3][:, :D], trainer.served[0])
    dr.status_check()


def test_save_incremental_refuses_an_untracked_table_by_name(dr, tmp_path):
    from deeprec_amd import checkpoint as ck
    m = Model(dr, 4)
    opt = make_opt(dr, "adagrad")
    m.v["bucket"].track_updates()
    with pytest.raises(dr.InvalidArgumentError, match="ck_mha.*not tracking"):
        ck.save_incremental(str(tmp_path / "d"), {"bucket": m.v["bucket"], "mh": m.v["mh_add"]})
    st = opt.checkpoint_variables({"mh": m.v["mh_add"]})
    with pytest.raises(dr.InvalidArgumentError, match="not tracking"):
        ck.save_incremental(str(tmp_path / "d"), st)
    assert m.v["bucket"].updated_count() == 0
