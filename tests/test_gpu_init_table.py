"""GPU: the EV init table (InitializerOption -> dr_ev_set_init_table, DESIGN
section 18).  With an init_option the initializer is run once for a
[default_value_dim, dim] table and every path that creates a key's row --
resolve / gather, the fused one-hot miss path, an apply that names a key no
lookup created, the tagged and XGMI owner sides -- starts key k from table row
k % K (a floor mod on the signed key).

Every comparison is bit-exact.  Two references, neither of which runs new
code: the table indexed on the host with Python's %, and a twin -- a
constant-initializer EV into which insert(keys, table[keys % K]) was called
for exactly the keys the test later creates, driven by the same calls (keys
and values are compared, not freq or version)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
KS = [1, 3, 4096]
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


def raw(t):
    """The tensor's bits (bf16 / fp32 / fp64 rows compared as integers)."""
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and torch.equal(raw(a), raw(b))


def _normal(seed):
    def init(shape):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(shape, generator=g, dtype=torch.float64) * 0.5
    return init


def make(dr, dim, K, dtype=torch.float32, no_perm=0.0, seed=None, **opt):
    """An EV whose keys start from a seeded random [K, dim] init table."""
    _N[0] += 1
    io = dr.InitializerOption(_normal(_N[0] if seed is None else seed), K, no_perm)
    o = dr.EmbeddingVariableOption(**opt).with_init_option(io)
    return dr.EmbeddingVariable("it_%d" % _N[0], dim, None, ev_option=o, device=DEV,
                                value_dtype=dtype, capacity=2048)


def twin_of(dr, ev, keys, no_perm=0.0, **opt):
    """Existing code only: a constant-initializer EV holding table[key % K]
    for `keys` (the keys the test goes on to create)."""
    _N[0] += 1
    o = dr.EmbeddingVariableOption(**opt) if opt else None
    tw = dr.EmbeddingVariable("it_tw_%d" % _N[0], ev.dim, no_perm, ev_option=o, device=DEV,
                              value_dtype=ev.value_dtype, capacity=2048)
    keys = np.unique(np.asarray(keys, dtype=np.int64))
    tw.insert(T(keys), ref_rows(ev, keys))
    return tw


def ref_rows(ev, keys):
    """table[key % K] with Python's % on Python ints (a floor mod)."""
    tab = ev.init_table
    K = tab.shape[0]
    idx = [int(k) % K for k in np.asarray(keys).reshape(-1).tolist()]
    return tab[T(np.asarray(idx, dtype=np.int64))]


def export(ev):
    k, v = ev.export()[:2]
    return k, v


def same_export(a, b):
    (ka, va), (kb, vb) = export(a), export(b)
    return torch.equal(ka, kb) and same(va, vb)


def edge_keys(K):
    return np.array([0, -1, -2, K, K + 1, I64_MIN, I64_MAX, 5, 5, 7 * K + 2, -K, -K - 1, 5],
                    dtype=np.int64)


def onehot_sp(dr, ids):
    B = ids.numel()
    ind = torch.stack([torch.arange(B, device=DEV), torch.zeros(B, dtype=torch.int64,
                                                                device=DEV)], 1)
    return dr.SparseTensor(ind, ids, (B, 1))


# ---------------------------------------------------------------------------
# 1. sparse_read on fresh keys
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dim,dtype", [(6, torch.float32), (128, torch.float32),
                                       (8, torch.bfloat16), (4, torch.float64)])
def test_sparse_read_fresh_keys(dr, dim, dtype, K):
    ev = make(dr, dim, K, dtype)
    assert ev.init_table.shape == (K, dim) and ev.init_table.dtype == dtype
    assert not ev.draws_defaults_per_call()
    keys = edge_keys(K)
    want = ref_rows(ev, keys)
    out = ev.sparse_read(T(keys))
    assert same(out, want)
    assert same(ev.sparse_read(T(keys)), want)       # stored, not drawn again
    k, v = export(ev)
    uk = np.unique(keys)
    assert k.cpu().numpy().tolist() == uk.tolist()
    assert same(v, ref_rows(ev, uk))
    dr.status_check()


# ---------------------------------------------------------------------------
# 2. order independence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 4096])
def test_initial_rows_do_not_depend_on_order(dr, K):
    rng = np.random.default_rng(K)
    keys = np.unique(rng.integers(I64_MIN, I64_MAX, 200, dtype=np.int64, endpoint=True))
    a, b = make(dr, 8, K, seed=900 + K), make(dr, 8, K, seed=900 + K)
    assert same(a.init_table, b.init_table)
    a.sparse_read(T(keys))
    perm = rng.permutation(keys)
    for part in np.array_split(perm, 7):
        batch = np.concatenate([part, rng.choice(perm, 9)])      # repeats, earlier keys
        b.sparse_read(T(batch))
    b.sparse_read(T(perm))
    assert same_export(a, b)
    assert same(export(a)[1], ref_rows(a, export(a)[0].cpu().numpy()))
    dr.status_check()


# ---------------------------------------------------------------------------
# 3. grouped multi-hot path
# ---------------------------------------------------------------------------
def _multihot(dr, rng, B, vocab):
    lens = rng.integers(0, 5, B)                               # bags of 0..4 ids
    rows = np.repeat(np.arange(B), lens)
    cols = np.concatenate([np.arange(n) for n in lens])
    ids = rng.choice(vocab, rows.shape[0])
    return dr.SparseTensor(T(np.stack([rows, cols], 1).astype(np.int64)), T(ids), (B, 4)), ids


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_grouped_multihot_matches_twin(dr, monkeypatch, combiner, train):
    from deeprec_amd import embedding_ops as eo
    rng = np.random.default_rng(31)
    B, D, K = 200, 16, 3
    vocab = np.concatenate([np.arange(-40, 60, dtype=np.int64),
                            np.array([I64_MIN, I64_MAX], dtype=np.int64)])
    sps, ids = zip(*[_multihot(dr, rng, B, vocab) for _ in range(3)])
    evs = [make(dr, D, K) for _ in range(3)]
    twins = [twin_of(dr, e, i) for e, i in zip(evs, ids)]
    grouped = []
    real = eo._prepare_group
    monkeypatch.setattr(eo, "_prepare_group",
                        lambda feats, *a, **k: (grouped.append(len(feats)), real(feats, *a, **k))[1])
    g = T(rng.standard_normal((B, 3 * D)).astype(np.float32))
    outs = []
    for tables in (evs, twins):
        if train:
            opt = dr.GradientDescentOptimizer(0.1)
            out = dr.embedding_lookup_sparse_multi(tables, list(sps), combiner=combiner)
            out.backward(g)
            opt.apply_gradients(tables)
        else:
            with torch.no_grad():
                out = dr.embedding_lookup_sparse_multi(tables, list(sps), combiner=combiner)
        outs.append(out.detach())
    assert grouped == [3, 3]                 # one grouped resolve per lookup, both sides
    assert same(outs[0], outs[1])
    for e, tw in zip(evs, twins):
        assert same_export(e, tw)
    dr.status_check()


# ---------------------------------------------------------------------------
# 4. fused one-hot: the miss path, then recorded rows + fused SGD
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["feature_major", "record_major"])
@pytest.mark.parametrize("K", [3, 4096])
def test_fused_onehot_matches_twin(dr, K, layout):
    from deeprec_amd import embedding_ops as eo
    from deeprec_amd.kv_variable_ops import PendingRowSlices
    rng = np.random.default_rng(K)
    F, B, D = 4, 128, 128
    known = rng.integers(-500, 500, (F, 400)).astype(np.int64)

    def batch(step):
        ids = np.stack([rng.choice(known[f], B) for f in range(F)])         # [F, B]
        new = rng.random((F, B)) < 0.3                                       # ~30 % new keys
        fresh = rng.integers(I64_MIN, I64_MAX, (F, B), dtype=np.int64, endpoint=True)
        return np.where(new, fresh, ids)

    batches = [batch(s) for s in range(4)]
    batches[0][0, :7] = edge_keys(K)[:7]
    evs = [make(dr, D, K) for _ in range(F)]
    twins = [twin_of(dr, evs[f], np.concatenate([b[f] for b in batches])) for f in range(F)]

    def sps(ids):
        if layout == "record_major":
            rec = T(np.ascontiguousarray(ids.T))                             # [B, F]
            return [onehot_sp(dr, rec[:, f]) for f in range(F)]
        fm = T(ids)                                                          # [F, B]
        return [onehot_sp(dr, fm[f]) for f in range(F)]

    sp0 = sps(batches[0])
    feats = [eo._Feature(evs[f], sp0[f].values, sp0[f].indices, B, None, "sum", None, onehot=True)
             for f in range(F)]
    assert eo._fused_onehot_ok(feats) and eo._rows_eligible(feats)
    if layout == "record_major":
        assert eo._record_major(feats) is not None
    ups = [T(rng.standard_normal((B, F * D)).astype(np.float32)) for _ in range(4)]
    results = []
    for tables in (evs, twins):
        outs = []
        with torch.no_grad():                       # fresh keys: ev_miss_kernel creates them
            outs.append(dr.embedding_lookup_sparse_multi(tables, sps(batches[0]), combiner="sum"))
        opt = dr.GradientDescentOptimizer(0.05)
        for s in range(1, 4):
            out = dr.embedding_lookup_sparse_multi(tables, sps(batches[s]), combiner="sum")
            out.backward(ups[s])
            pend = [e.pending_grads[-1] for e in tables]
            assert all(isinstance(p, PendingRowSlices) and p.fusable() for p in pend)
            opt.apply_gradients(tables, global_step=s)
            assert all(p._pending.applied for p in pend)     # backward fused into KV SGD
            outs.append(out.detach())
        results.append(outs)
    for f in range(F):
        want = ref_rows(evs[f], batches[0][f])
        assert same(results[0][0].reshape(B, F, D)[:, f, :], want)
    for x, y in zip(*results):
        assert same(x, y)
    for e, tw in zip(evs, twins):
        assert same_export(e, tw)
    dr.status_check()


# ---------------------------------------------------------------------------
# 5. apply_gradients creates the key
# ---------------------------------------------------------------------------
def _optimizer(dr, name):
    return {"sgd": lambda: dr.GradientDescentOptimizer(0.1),
            "adagrad": lambda: dr.AdagradOptimizer(0.1, initial_accumulator_value=0.3),
            "adam": lambda: dr.AdamOptimizer(0.01)}[name]()


@pytest.mark.parametrize("K", [3, 4096])
@pytest.mark.parametrize("dim", [6, 8])
@pytest.mark.parametrize("opt_name,dtype", [("sgd", torch.float32), ("adagrad", torch.float32),
                                            ("adam", torch.float32), ("sgd", torch.bfloat16),
                                            ("adagrad", torch.bfloat16)])
def test_apply_creates_the_key(dr, opt_name, dtype, dim, K):
    """Gradients for keys no lookup created: the apply kernel's first touch of
    the primary column copies the key's table row, the slots their constant."""
    rng = np.random.default_rng(dim * 10 + K)
    k1 = np.unique(np.concatenate([edge_keys(K), rng.integers(-10**12, 10**12, 70)]))
    k2 = np.unique(np.concatenate([k1[::3], rng.integers(-10**12, 10**12, 40)]))
    ev = make(dr, dim, K, dtype)
    tw = twin_of(dr, ev, np.concatenate([k1, k2]))
    for table in (ev, tw):
        opt = _optimizer(dr, opt_name)
        for step, keys in enumerate((k1, k2)):
            g = T(np.random.default_rng(step).standard_normal((keys.size, dim)).astype(np.float32))
            table.pending_grads.append(dr.IndexedSlices(g, T(keys)))
            opt.apply_gradients([table], global_step=step + 1)
        table._test_slots = [s for s in opt._slots(table) or () if s is not None] \
            if opt_name != "sgd" else []
    assert same_export(ev, tw)
    assert len(ev._test_slots) == {"sgd": 0, "adagrad": 1, "adam": 2}[opt_name]
    for s, ts in zip(ev._test_slots, tw._test_slots):
        assert s.init_table is None
        assert same_export(s, ts)
    # and the values are not the no-permission row: they moved from the table rows
    k, v = export(ev)
    assert not same(v, torch.zeros_like(v))
    dr.status_check()


# ---------------------------------------------------------------------------
# 6. filter and read-only: the default row keeps its second role
# ---------------------------------------------------------------------------
def test_counter_filter_serves_the_no_permission_row(dr):
    """CounterFilter(filter_freq=3): a lookup that finds freq < 3 serves the
    default_value_no_permission row and counts; the first lookup that finds
    freq >= 3 creates the row from the init table.  By the reference's rule
    (the frequency is tested before it is added to, embedding_filter.h:296-320,
    which the oracle and the existing parity tests pin) lookups 1-3 find 0, 1
    and 2, so the table row arrives with lookup 4; a constant-initializer twin
    is admitted at the same lookup."""
    D, K = 8, 3
    filt = dict(filter_option=dr.CounterFilter(filter_freq=3))
    ev = make(dr, D, K, no_perm=0.25, **filt)
    tw = dr.EmbeddingVariable("it_cf_tw", D, 0.5, ev_option=dr.EmbeddingVariableOption(**filt),
                              device=DEV)
    keys = np.array([11, -4, I64_MIN, 7], dtype=np.int64)
    quarter = torch.full((keys.size, D), 0.25, device=DEV)
    for look in (1, 2, 3):
        assert same(ev.sparse_read(T(keys)), quarter), look
        assert same(tw.sparse_read(T(keys)), torch.full_like(quarter, 0.5)), look
    assert same(ev.sparse_read(T(keys)), ref_rows(ev, keys))
    assert same(tw.sparse_read(T(keys)), torch.full_like(quarter, 0.5))     # its constant row
    assert same(ev.sparse_read(T(keys)), ref_rows(ev, keys))
    # read-only: an absent key reads the 0.25 row and nothing is created
    absent = np.array([1001, -1002, I64_MAX], dtype=np.int64)
    n0 = int(ev.total_count()[0])
    q3 = torch.full((absent.size, D), 0.25, device=DEV)
    assert same(ev.sparse_read(T(absent), read_only=True), q3)
    with dr.read_only_lookups():
        out = dr.embedding_lookup_sparse(ev, onehot_sp(dr, T(absent)), combiner="sum")
        assert same(ev.sparse_read(T(absent)), q3)
    assert same(out, q3)
    assert int(ev.total_count()[0]) == n0
    dr.status_check()


def test_read_only_miss_without_filter(dr):
    ev = make(dr, 8, 3, no_perm=0.25)
    ev.sparse_read(T(np.array([1, 2], dtype=np.int64)))
    absent = T(np.array([50, -50], dtype=np.int64))
    assert same(ev.sparse_read(absent, read_only=True), torch.full((2, 8), 0.25, device=DEV))
    assert int(ev.total_count()[0]) == 2
    assert same(ev.sparse_read(absent), ref_rows(ev, [50, -50]))    # then created from the table


# ---------------------------------------------------------------------------
# 7. per-call override
# ---------------------------------------------------------------------------
def test_ev_init_value_wins(dr):
    ev = make(dr, 8, 3)
    v = torch.arange(8, dtype=torch.float32, device=DEV) + 0.5
    keys = T(np.array([9, -9], dtype=np.int64))
    assert same(ev.sparse_read(keys, ev_init_value=v), v.expand(2, 8))
    assert same(ev.sparse_read(keys), v.expand(2, 8))             # stored
    assert same(ev.sparse_read(T(np.array([10], dtype=np.int64))), ref_rows(ev, [10]))


# ---------------------------------------------------------------------------
# 8. tier transparency
# ---------------------------------------------------------------------------
def test_tiered_ev_matches_untiered_twin(dr):
    D, K, N = 8, 3, 200
    rng = np.random.default_rng(8)
    keys = np.unique(rng.integers(-10**9, 10**9, N + 50))[:N]
    rng.shuffle(keys)
    a = make(dr, D, K, seed=77, evict_option=dr.KeyBudgetEvict(N // 2, "lru", steps_to_live=1000),
             storage_option=dr.StorageOption(dr.StorageType.HBM_DRAM))
    b = make(dr, D, K, seed=77, evict_option=dr.GlobalStepEvict(1000))
    assert same(a.init_table, b.init_table)
    fresh = np.arange(10**10, 10**10 + 20, dtype=np.int64)
    mix = np.concatenate([keys[50:150], fresh])              # demoted, resident and brand new
    outs = []
    for ev in (a, b):
        opt = dr.GradientDescentOptimizer(0.1)
        o = []
        for step, ks in enumerate((keys, keys[N // 2:])):
            g = T(np.random.default_rng(step).standard_normal((ks.size, D)).astype(np.float32))
            out = dr.embedding_lookup_sparse(ev, onehot_sp(dr, T(ks)), combiner="sum")
            out.backward(g)
            opt.apply_gradients([ev], global_step=step + 1)
            o.append(out.detach())
        if ev is a:
            assert ev.demote_to() == N // 2 and ev.tier_count() == N // 2
        with torch.no_grad():
            o.append(dr.embedding_lookup_sparse(ev, onehot_sp(dr, T(mix)), combiner="sum"))
        outs.append(o)
    for x, y in zip(*outs):
        assert same(x, y)
    # the demoted keys came back trained, not re-initialised
    assert not same(outs[0][2][:50], ref_rows(a, mix[:50]))
    assert same(outs[0][2][100:], ref_rows(a, fresh))
    assert same_export(a, b)
    dr.status_check()


# ---------------------------------------------------------------------------
# 9. capture
# ---------------------------------------------------------------------------
def test_captured_lookup_creates_keys_from_the_table(dr):
    F, B, D, K = 2, 64, 16, 3
    evs = [make(dr, D, K) for _ in range(F)]
    for e in evs:
        e.reserve(4 * B)
    ids = T(np.arange(F * B, dtype=np.int64).reshape(F, B))
    sps = [onehot_sp(dr, ids[f]) for f in range(F)]
    with torch.no_grad():
        dr.embedding_lookup_sparse_multi(evs, sps, combiner="sum")       # warm-up, eager
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = dr.embedding_lookup_sparse_multi(evs, sps, combiner="sum")
    new = np.random.default_rng(9).integers(I64_MIN, -1, (F, B), dtype=np.int64)   # all new
    ids.copy_(T(new))
    g.replay()
    torch.cuda.synchronize()
    dr.status_check()
    for f in range(F):
        assert same(out.reshape(B, F, D)[:, f, :], ref_rows(evs[f], new[f]))
        k, v = export(evs[f])
        sel = torch.isin(k, T(new[f]))
        assert int(sel.sum()) == np.unique(new[f]).size
        assert same(v[sel], ref_rows(evs[f], k[sel].cpu().numpy()))


# ---------------------------------------------------------------------------
# 10. sharded owner paths
# ---------------------------------------------------------------------------
def test_tagged_resolve_and_gather(dr):
    from deeprec_amd._lib import check, lib, ptr, stream_handle, workspace
    D, n = 8, 64
    evs = [make(dr, D, 3), make(dr, D, 4096)]
    rng = np.random.default_rng(10)
    keys = np.concatenate([edge_keys(3)[:7], rng.integers(-10**6, 10**6, n - 7)]).astype(np.int64)
    tags = rng.integers(0, 2, n).astype(np.int32)
    h = (C.c_void_p * 2)(*[e.handle.value for e in evs])
    rows = torch.empty(n, dtype=torch.int64, device=DEV)
    out = torch.empty((n, D), dtype=torch.float32, device=DEV)
    wsb = lib().dr_ev_resolve_workspace_size(n)
    ws = workspace(wsb, DEV)
    kd, td = T(keys), T(tags)
    check(lib().dr_ev_resolve_tagged(h, 2, ptr(kd), ptr(td), n, None, None, None, ptr(rows),
                                     ptr(ws), wsb, stream_handle(DEV)))
    check(lib().dr_ev_gather_tagged(h, 2, ptr(td), ptr(rows), n, None, ptr(out),
                                    stream_handle(DEV)))
    torch.cuda.synchronize()
    dr.status_check()
    assert int(rows.min()) >= 0
    for t in range(2):
        m = tags == t
        assert same(out[T(m)], ref_rows(evs[t], keys[m]))
        assert same(export(evs[t])[1], ref_rows(evs[t], np.unique(keys[m])))


def test_xgmi_owner_side_world_1(dr):
    from deeprec_amd.sharded import XgmiShardedLookup
    F, B, D = 2, 64, 8
    evs = [make(dr, D, 3), make(dr, D, 4096)]
    eng = XgmiShardedLookup(evs, 1, 0, B, torch.device(DEV))
    ids = np.random.default_rng(12).integers(-10**6, 10**6, (F, B)).astype(np.int64)
    ids[:, :7] = edge_keys(3)[:7]
    with torch.no_grad():
        out = eng.forward(T(ids))
    torch.cuda.synchronize()
    dr.status_check()
    for f in range(F):
        assert same(out.reshape(B, F, D)[:, f, :], ref_rows(evs[f], ids[f]))
        assert same(export(evs[f])[1], ref_rows(evs[f], np.unique(ids[f])))


# ---------------------------------------------------------------------------
# 11. ABI refusals
# ---------------------------------------------------------------------------
def test_set_init_table_refusals(dr):
    from deeprec_amd._lib import INVALID_ARGUMENT, lib, stream_handle
    L = lib()
    st = stream_handle(DEV)
    plain = dr.EmbeddingVariable("it_plain", 8, 0.5, device=DEV)
    assert L.dr_ev_init_table_rows(plain.handle) == 1 and not L.dr_ev_init_table(plain.handle)
    assert plain.init_table is None
    tab = torch.arange(24, dtype=torch.float32).reshape(3, 8).contiguous()
    for rows in (0, -1, (1 << 20) + 1):
        assert L.dr_ev_set_init_table(plain.handle, tab.data_ptr(), rows, st) == INVALID_ARGUMENT
    assert L.dr_ev_set_init_table(None, tab.data_ptr(), 3, st) == INVALID_ARGUMENT
    assert L.dr_ev_set_init_table(plain.handle, None, 3, st) == INVALID_ARGUMENT
    assert L.dr_ev_init_table_rows(plain.handle) == 1
    # an empty key space takes a table ...
    assert L.dr_ev_set_init_table(plain.handle, tab.data_ptr(), 3, st) == 0
    assert L.dr_ev_init_table_rows(plain.handle) == 3 and L.dr_ev_init_table(plain.handle)
    assert same(plain.sparse_read(T(np.array([-1, 4], dtype=np.int64))), tab[[2, 1]].to(DEV))
    # ... and refuses one once it holds a key; the table stays as it was
    other = (tab + 100).contiguous()
    assert L.dr_ev_set_init_table(plain.handle, other.data_ptr(), 3, st) == INVALID_ARGUMENT
    assert L.dr_last_error()
    assert L.dr_ev_init_table_rows(plain.handle) == 3
    assert same(plain.sparse_read(T(np.array([5, 6], dtype=np.int64))), tab[[2, 0]].to(DEV))
    # inside stream capture
    fresh = dr.EmbeddingVariable("it_cap", 8, 0.5, device=DEV)
    x = torch.zeros(4, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = x + 1
        rc = L.dr_ev_set_init_table(fresh.handle, tab.data_ptr(), 3, stream_handle(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert float(y.sum()) == 4.0
    assert rc == INVALID_ARGUMENT and L.dr_ev_init_table_rows(fresh.handle) == 1


def test_python_validation(dr):
    with pytest.raises(dr.InvalidArgumentError):
        dr.InitializerOption(default_value_dim=0)
    with pytest.raises(dr.InvalidArgumentError):
        dr.InitializerOption(default_value_dim=(1 << 20) + 1)
    bad = dr.EmbeddingVariableOption().with_init_option(
        dr.InitializerOption(lambda s: torch.zeros(5, 8), 4))
    with pytest.raises(dr.InvalidArgumentError):
        dr.EmbeddingVariable("it_bad", 8, None, ev_option=bad, device=DEV)
    # a constant is broadcast; the EV's own initializer= is used when the option has none
    calls = []

    def ini(shape):
        calls.append(tuple(shape))
        return torch.ones(shape) * 2.0

    o = dr.EmbeddingVariableOption()
    o.init_option = dr.InitializerOption(None, 5, 0.25)         # the attribute, set directly
    ev = dr.EmbeddingVariable("it_own", 8, ini, ev_option=o, device=DEV)
    assert calls == [(5, 8)]
    assert same(ev.sparse_read(T(np.array([3], dtype=np.int64))), torch.full((1, 8), 2.0, device=DEV))
    assert calls == [(5, 8)]                       # never called per lookup
    c = dr.EmbeddingVariable("it_const", 8, None, device=DEV, ev_option=dr.EmbeddingVariableOption(
        ).with_init_option(dr.InitializerOption(1.5, 2)))
    assert same(c.init_table, torch.full((2, 8), 1.5, device=DEV))
    # without an init_option a callable initializer keeps its per-call draw
    legacy = dr.EmbeddingVariable("it_legacy", 8, ini, device=DEV)
    assert legacy.draws_defaults_per_call() and legacy.init_table is None
    legacy.sparse_read(T(np.array([1, 2], dtype=np.int64)))
    assert calls[-1] == (2, 8)
