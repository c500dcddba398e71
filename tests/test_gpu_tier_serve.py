"""GPU: pooled read-only lookups served from the host-DRAM tier in place
(read_only_lookups(serve_tier=True)).

The contract is section 16's transparency: inside such a block every pooled
read-only lookup of a tiered EV returns, bit for bit, what the same call
returns on an untiered, unbudgeted twin that saw the same history -- and
neither tier changes: export() of the primary and of the slot EV, the host
store's content and tier_count() are compared before and after every serving
call.  No tolerance appears anywhere.

Tiny shapes: capacity=1 EVs, batches of 64, values and gradients multiples of
0.5 (exact in bf16 too), keys from ev_lifecycle.universe.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ev_lifecycle as L
import tier_serve_walk as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I64MIN, I64MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
SPECIAL = np.array([-1, 0, I64MIN, I64MAX], np.int64)
TORCH_DT = {"float32": torch.float32, "bfloat16": torch.bfloat16}
B = 64


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    return deeprec_amd


@pytest.fixture(scope="module")
def uni():
    return L.universe(5)


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def bits(t):
    t = t.detach()
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy()
    return t.contiguous().view(torch.int32).cpu().numpy()


def snap(ev):
    k, v, ve, fr = ev.export()
    return k.cpu().numpy(), bits(v), ve.cpu().numpy(), fr.cpu().numpy()


def same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, i, x.shape, y.shape)
        np.testing.assert_array_equal(x, y, err_msg="%s: field %d" % (what, i))


def tier_state(ev):
    p = ev._primary or ev
    if p._tier is None:         # (no demotion yet: there is no store)
        return []
    with p._lock:
        k, vals, ve, fr, cm = p._tier_export()
    return [k, ve, fr, cm] + [v for v in vals if v is not None]


_N = [0]


def make(dr, tiered, dim=8, dtype="float32", filter_freq=0, init_option=None):
    """A tiered EV, or its twin: untiered and unbudgeted, otherwise the same."""
    _N[0] += 1
    evict = dr.KeyBudgetEvict(1 << 20, "lru", steps_to_live=50) if tiered \
        else dr.GlobalStepEvict(50)
    opt = dr.EmbeddingVariableOption(
        evict_option=evict,
        filter_option=dr.CounterFilter(filter_freq) if filter_freq else None,
        storage_option=dr.StorageOption(dr.StorageType.HBM_DRAM) if tiered else None)
    if init_option is not None:
        opt.init_option = init_option
    return dr.EmbeddingVariable("serve_%d_%s" % (_N[0], "a" if tiered else "b"), dim, L.DEFAULT,
                                ev_option=opt, device=DEV, value_dtype=TORCH_DT[dtype],
                                capacity=1)


def train(dr, opt, ev, keys, step, seed=0):
    """One step: the lookup of `keys` (duplicates and all), then the optimizer
    on the distinct keys with integer gradients and global_step = step."""
    ev.sparse_read(T(keys))
    u = np.unique(keys)
    g = np.random.default_rng([seed, 8, step]).integers(-2, 3, (u.size, ev.dim))
    ev.pending_grads.append(dr.IndexedSlices(T(g.astype(np.float32)), T(u)))
    opt.apply_gradients([ev], global_step=step)


def pairs(dr, uni, n, keys=None, keep=70, steps=2, **kw):
    """n tiered EVs and their twins, trained alike on `keys` (default: 220 of
    the universe and the four special keys), then each tiered one demoted down
    to `keep` keys in HBM.  Returns (As, Bs, per-EV tier keys, per-EV HBM keys)."""
    opt = dr.GradientDescentOptimizer(L.LR)
    As, Bs = [make(dr, True, **kw) for _ in range(n)], [make(dr, False, **kw) for _ in range(n)]
    tks, hks = [], []
    for i, (a, b) in enumerate(zip(As, Bs)):
        ks = np.concatenate([uni.keys[60 * i:60 * i + 220], SPECIAL]) if keys is None else keys
        ks = np.unique(ks)
        for step in range(steps):
            # (the special keys in the first step only: the coldest by LRU, so demoted)
            batch = ks if step == 0 else ks[~np.isin(ks, SPECIAL)]
            for ev in (a, b):
                train(dr, opt, ev, np.concatenate([batch, batch[:17]]), step, seed=i)
        assert a.demote_to(keep) == ks.size - keep
        tk = tier_state(a)[0]
        assert np.isin(SPECIAL, tk).all() or keys is not None
        tks.append(tk)
        hks.append(ks[~np.isin(ks, tk)])
    return As, Bs, tks, hks


NEVER = np.arange(1 << 41, (1 << 41) + 64, dtype=np.int64)


def mix(rng, tk, hk, n, special=True):
    """n ids: about half served by the tier, the rest from HBM and never seen,
    duplicates included, the special keys first."""
    ids = np.concatenate([rng.choice(tk, n // 2), rng.choice(hk, n // 4),
                          rng.choice(NEVER, n - n // 2 - n // 4)])
    ids = rng.permutation(ids)
    if special:
        ids[:4] = SPECIAL
    return ids.astype(np.int64)


def onehot_sp(dr, ids):
    n = ids.numel() if torch.is_tensor(ids) else len(ids)
    ind = T(np.stack([np.arange(n), np.zeros(n, np.int64)], 1))
    return dr.SparseTensor(ind, ids if torch.is_tensor(ids) else T(ids), (n, 1))


def bag_sp(dr, rng, ids_of, nbags=B, weights=False):
    """nbags bags of 0..5 ids with repeats inside and across bags."""
    lens = rng.integers(0, 6, nbags)
    lens[:3] = (0, 5, 1)
    rows = np.repeat(np.arange(nbags), lens)
    cols = np.concatenate([np.arange(n) for n in lens]).astype(np.int64)
    vals = ids_of(int(lens.sum()))
    start = np.cumsum(lens) - lens
    for b in np.nonzero(lens >= 3)[0]:
        vals[start[b] + 2] = vals[start[b]]
    ind = T(np.stack([rows, cols], 1))
    sp = dr.SparseTensor(ind, T(vals), (nbags, 5))
    if not weights:
        return sp, None
    w = rng.integers(1, 5, vals.size).astype(np.float32) * 0.5
    return sp, dr.SparseTensor(ind, T(w), (nbags, 5))


def serve_both(dr, As, Bs, call, watch=None):
    """call(evs) on the tiered EVs inside read_only_lookups(serve_tier=True) and
    on the twins inside read_only_lookups(): bit-equal outputs, and nothing of
    the tiered EVs (and of `watch`, e.g. their slot EVs) changed."""
    watch = list(As) + list(watch or [])
    watch = [e for e in watch if hasattr(e, "export")]
    prim = {id(e._primary or e): (e._primary or e) for e in watch}.values()
    before = [(snap(e), e.tier_count()) for e in watch]
    tier0 = [tier_state(p) for p in prim]
    with dr.read_only_lookups(serve_tier=True):
        oa = call(As)
    with dr.read_only_lookups():
        ob = call(Bs)
    assert oa.dtype == ob.dtype and oa.shape == ob.shape
    assert (oa.grad_fn is None) == (ob.grad_fn is None)     # (a DenseTable feature has one)
    np.testing.assert_array_equal(bits(oa), bits(ob))
    for e, (s, n) in zip(watch, before):
        same(snap(e), s, "export() of %s after serving" % e.name)
        assert e.tier_count() == n
    for p, t0 in zip(prim, tier0):
        same(tier_state(p), t0, "the host tier of %s after serving" % p.name)
    dr.status_check()
    return oa


def default_bits(ev, like=None):
    """The EV's default row as the bits of an output of `like`'s dtype."""
    d = ev.default_value.reshape(1, ev.dim)
    return bits(d if like is None else d.to(like.dtype))


# ---------------------------------------------------------------------------
# 1. the fused one-hot route
# ---------------------------------------------------------------------------
FUSED = [("float32", 4, None), ("float32", 16, None), ("float32", 128, None),
         ("float32", 256, None), ("bfloat16", 8, None), ("bfloat16", 64, None),
         ("bfloat16", 8, torch.bfloat16), ("bfloat16", 64, torch.bfloat16)]


@pytest.mark.parametrize("dtype,dim,out_dtype", FUSED,
                         ids=["%s-%d-%s" % (d, n, "bf16out" if o else "f32out")
                              for d, n, o in FUSED])
def test_fused_onehot_route_equals_twin(dr, uni, monkeypatch, dtype, dim, out_dtype):
    import deeprec_amd.embedding_ops as eo
    As, Bs, tks, hks = pairs(dr, uni, 3, dim=dim, dtype=dtype)
    rng = np.random.default_rng(dim)
    ids = np.stack([mix(rng, tks[t], hks[t], B) for t in range(3)], 1)       # [B, T]
    patched = []
    real = dr._lib.lib().dr_ev_overlay_patch_onehot
    monkeypatch.setattr(dr._lib.lib(), "dr_ev_overlay_patch_onehot",
                        lambda *a: patched.append(a[2]) or real(*a))
    # record-major: the features are the columns of one [B, T] id matrix, read in place
    rec = T(ids)
    out = serve_both(dr, As, Bs, lambda evs: dr.embedding_lookup_sparse_multi(
        evs, [onehot_sp(dr, rec[:, t]) for t in range(3)], combiner="sum", out_dtype=out_dtype))
    assert len(patched) == 1 and patched[0] >= B       # the fused route, one patch launch
    # feature-major ids
    fm = T(np.ascontiguousarray(ids.T))
    out2 = serve_both(dr, As, Bs, lambda evs: dr.embedding_lookup_sparse_multi(
        evs, [onehot_sp(dr, fm[t]) for t in range(3)], combiner="mean", out_dtype=out_dtype))
    np.testing.assert_array_equal(bits(out), bits(out2))
    assert len(patched) == 2
    # tier ids read stored rows, never-seen ids the default
    o = bits(out).reshape(B, 3, dim)
    for t in range(3):
        d = default_bits(As[t], out)
        assert (o[np.isin(ids[:, t], NEVER), t] == d).all()
        assert (o[np.isin(ids[:, t], tks[t]), t] != d).any()
    if dtype == "float32":
        # the other association order (the layer below the public lookups reaches it)
        def seq(evs):
            feats = [eo._Feature(e, fm[t], eo._seg_of(onehot_sp(dr, fm[t])), B, None, "sum", None,
                                 onehot=True) for t, e in enumerate(evs)]
            return eo._run_readonly(feats, eo.ORDER_SEQ, None)
        serve_both(dr, As, Bs, seq)
        assert len(patched) == 3


@pytest.mark.parametrize("case", ["dim6", "dim260", "33features"])
def test_shapes_off_the_fused_route_equal_twin(dr, uni, monkeypatch, case):
    dim = {"dim6": 6, "dim260": 260}.get(case, 8)
    As, Bs, tks, hks = pairs(dr, uni, 3, dim=dim)
    n = 33 if case == "33features" else 3
    assert n <= dr._lib.MAX_GROUP + 1
    rng = np.random.default_rng(len(case))
    ids = [mix(rng, tks[t % 3], hks[t % 3], B) for t in range(n)]
    calls = []
    lib = dr._lib.lib()
    real_p, real_r = lib.dr_ev_overlay_patch_onehot, lib.dr_ev_overlay_resolve
    monkeypatch.setattr(lib, "dr_ev_overlay_patch_onehot",
                        lambda *a: calls.append("patch") or real_p(*a))
    monkeypatch.setattr(lib, "dr_ev_overlay_resolve",
                        lambda *a: calls.append("resolve") or real_r(*a))
    out = serve_both(dr, As, Bs, lambda evs: dr.embedding_lookup_sparse_multi(
        [evs[t % 3] for t in range(n)], [onehot_sp(dr, k) for k in ids], combiner="sum"))
    assert calls == ["resolve"] * (2 if n == 33 else 1), calls      # 33 features: two chunks
    o = bits(out).reshape(B, n, dim)
    for t in range(n):
        d = default_bits(As[t % 3])
        assert (o[np.isin(ids[t], NEVER), t] == d).all()
        assert (o[np.isin(ids[t], tks[t % 3]), t] != d).any()


# ---------------------------------------------------------------------------
# 2. the resolve -> pool route
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pooled(dr, uni):
    return pairs(dr, uni, 2, dim=8)


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("variant", ["plain", "weights", "max_norm"])
def test_bags_equal_twin(dr, pooled, combiner, variant):
    As, Bs, tks, hks = pooled
    rng = np.random.default_rng([len(combiner), len(variant)])
    sp, spw = bag_sp(dr, rng, lambda n: mix(rng, tks[0], hks[0], max(n, 8))[:n],
                     weights=variant == "weights")
    out = serve_both(dr, As[:1], Bs[:1], lambda evs: dr.embedding_lookup_sparse(
        evs[0], sp, spw, combiner=combiner, max_norm=1.5 if variant == "max_norm" else None))
    if variant != "weights":                 # (an empty weighted bag divides by its zero weight)
        assert (bits(out)[0] == 0).all()     # bag 0 is empty


@pytest.mark.parametrize("dtype,out_dtype", [("bfloat16", None), ("bfloat16", torch.bfloat16)])
def test_bf16_bags_equal_twin(dr, uni, dtype, out_dtype):
    As, Bs, tks, hks = pairs(dr, uni, 2, dim=16, dtype=dtype)
    rng = np.random.default_rng(3)
    sps = [bag_sp(dr, rng, lambda n, t=t: mix(rng, tks[t], hks[t], max(n, 8))[:n])[0]
           for t in range(2)]
    serve_both(dr, As, Bs, lambda evs: dr.embedding_lookup_sparse_multi(
        evs, sps, combiner="mean", out_dtype=out_dtype))


def test_safe_lookup_with_a_tier_resident_default_id(dr, uni):
    # (positive keys: the safe lookup prunes negative ids)
    As, Bs, tks, hks = pairs(dr, uni, 1, keys=np.arange(1000, 1220, dtype=np.int64))
    rng = np.random.default_rng(11)
    tk = tks[0]
    default_id = int(tk[0])

    def ids_of(n):
        v = mix(rng, tk, hks[0], max(n, 8), special=False)[:n]
        v[::7] = -5         # negative ids are pruned
        return v
    sp, _ = bag_sp(dr, rng, ids_of)
    out = serve_both(dr, As[:1], Bs[:1], lambda evs: dr.safe_embedding_lookup_sparse(
        evs[0], sp, combiner="mean", default_id=default_id))
    # the empty bag reads the default id's stored row, out of the tier
    with dr.read_only_lookups():
        want = Bs[0].sparse_read(T(np.array([default_id], np.int64)))
    np.testing.assert_array_equal(bits(out)[0], bits(want)[0])
    assert (bits(out)[0] != default_bits(As[0])).any()
    serve_both(dr, As[:1], Bs[:1], lambda evs: dr.safe_embedding_lookup_sparse(
        evs[0], sp, combiner="sum"))


def test_two_features_over_one_ev_and_a_dense_table(dr, pooled):
    As, Bs, tks, hks = pooled
    rng = np.random.default_rng(12)
    dense = dr.DenseTable(T(rng.integers(-4, 5, (50, 8)).astype(np.float32) * 0.5))
    sp0, _ = bag_sp(dr, rng, lambda n: mix(rng, tks[0], hks[0], max(n, 8))[:n])
    sp1, _ = bag_sp(dr, rng, lambda n: mix(rng, tks[0], hks[0], max(n, 8))[:n])
    sp2, _ = bag_sp(dr, rng, lambda n: mix(rng, tks[1], hks[1], max(n, 8))[:n])
    spd, _ = bag_sp(dr, rng, lambda n: rng.integers(0, 50, n))
    serve_both(dr, As, Bs, lambda evs: dr.embedding_lookup_sparse_multi(
        [evs[0], evs[0], evs[1]], [sp0, sp1, sp2], combiner="mean"))
    serve_both(dr, As + [dense], Bs + [dense], lambda evs: dr.embedding_lookup_sparse_multi(
        [evs[0], evs[2], evs[1], evs[0]], [sp0, spd, sp2, sp1], combiner="sum"))
    # one-hot features mixed with the dense table: the EVs take the fused route
    ids = [mix(rng, tks[t], hks[t], B) for t in range(2)]
    sps = [onehot_sp(dr, ids[0]), onehot_sp(dr, rng.integers(0, 50, B)), onehot_sp(dr, ids[1])]
    serve_both(dr, As + [dense], Bs + [dense], lambda evs: dr.embedding_lookup_sparse_multi(
        [evs[0], evs[2], evs[1]], sps, combiner="sum"))


def test_embedding_stack_equals_twin(dr, pooled):
    As, Bs, tks, hks = pooled
    rng = np.random.default_rng(13)
    x0 = T(rng.integers(-4, 5, (B, 8)).astype(np.float32))
    ids = [mix(rng, tks[t], hks[t], B) for t in range(2)]
    stack = dr.embedding_ops.embedding_stack
    out = serve_both(dr, As, Bs, lambda evs: stack(x0, evs, [onehot_sp(dr, k) for k in ids]))
    assert tuple(out.shape) == (B, 3, 8)
    sps = [bag_sp(dr, rng, lambda n, t=t: mix(rng, tks[t], hks[t], max(n, 8))[:n])[0]
           for t in range(2)]
    serve_both(dr, As, Bs, lambda evs: stack(x0, evs, sps, combiner="sum"))


# ---------------------------------------------------------------------------
# 3. keys and admission
# ---------------------------------------------------------------------------
def test_special_keys_are_served_from_the_tier(dr, pooled):
    As, Bs, tks, hks = pooled
    assert np.isin(SPECIAL, tks[0]).all()
    ids = np.tile(SPECIAL, B // 4)
    out = serve_both(dr, As[:1], Bs[:1], lambda evs: dr.embedding_lookup_sparse(
        evs[0], onehot_sp(dr, ids), combiner="sum"))
    o = bits(out)
    np.testing.assert_array_equal(o[:4], o[4:8])
    assert all((o[i] != default_bits(As[0])).any() for i in range(4))
    # ... and through the pool route: bags of all four
    ind = T(np.stack([np.repeat(np.arange(B // 4), 4), np.tile(np.arange(4), B // 4)], 1))
    sp = dr.SparseTensor(ind, T(ids), (B // 4, 4))
    serve_both(dr, As[:1], Bs[:1],
               lambda evs: dr.embedding_lookup_sparse(evs[0], sp, combiner="mean"))


def test_counter_ev_below_threshold_reads_the_default(dr, uni):
    opt = dr.GradientDescentOptimizer(L.LR)
    a, b = make(dr, True, filter_freq=2), make(dr, False, filter_freq=2)
    ks = uni.keys[:200]
    for step in range(2):
        for ev in (a, b):
            train(dr, opt, ev, ks, step)
    once = uni.keys[300:340]
    for ev in (a, b):
        ev.sparse_read(T(once))                  # one sighting: below filter_freq
    assert a.demote_to(0) == 240
    k, ve, fr, cm = tier_state(a)[:4]
    assert (fr[np.isin(k, once)] == 1).all() and (fr[np.isin(k, ks)] >= 2).all()
    ids = np.concatenate([once[:24], ks[:40]])
    out = serve_both(dr, [a], [b], lambda evs: dr.embedding_lookup_sparse(
        evs[0], onehot_sp(dr, ids), combiner="sum"))
    o = bits(out)
    assert (o[:24] == default_bits(a)).all()     # stored, but not admitted: the default
    assert (o[24:] != default_bits(a)).any(1).sum() > 30
    rng = np.random.default_rng(5)
    sp, _ = bag_sp(dr, rng, lambda n: rng.choice(np.concatenate([once, ks, NEVER[:20]]), n))
    serve_both(dr, [a], [b], lambda evs: dr.embedding_lookup_sparse(evs[0], sp, combiner="sum"))


def test_slot_column_with_a_clear_bit(dr, uni):
    ada = dr.AdagradOptimizer(L.LR)
    sgd = dr.GradientDescentOptimizer(L.LR)
    a, b = make(dr, True), make(dr, False)
    sa, sb = [e.slot("Adagrad", ada.init_acc) for e in (a, b)]
    touched, untouched = uni.keys[:120], uni.keys[120:200]
    for step in range(2):
        for ev in (a, b):
            train(dr, ada, ev, touched, step)        # the slot column is touched
            train(dr, sgd, ev, untouched, step)      # ... and here it is not
    assert a.demote_to(0) == 200
    k, ve, fr, cm = tier_state(a)[:4]
    assert ((cm[np.isin(k, untouched)] >> 1) & 1 == 0).all()
    assert ((cm[np.isin(k, touched)] >> 1) & 1 == 1).all()
    ids = np.concatenate([untouched[:32], touched[:32]])
    out = serve_both(dr, [sa], [sb], lambda evs: dr.embedding_lookup_sparse(
        evs[0], onehot_sp(dr, ids), combiner="sum"), watch=[a])
    o = bits(out)
    assert (o[:32] == default_bits(sa)).all()
    assert (o[32:] != default_bits(sa)).any()
    rng = np.random.default_rng(6)
    sp, _ = bag_sp(dr, rng, lambda n: rng.choice(ids, n))
    serve_both(dr, [sa], [sb], lambda evs: dr.embedding_lookup_sparse(
        evs[0], sp, combiner="mean"), watch=[a])
    # the primary and its slot as two features of one lookup
    serve_both(dr, [a, sa], [b, sb], lambda evs: dr.embedding_lookup_sparse_multi(
        evs, [onehot_sp(dr, ids), onehot_sp(dr, ids[::-1].copy())], combiner="sum"))


def test_init_option_hits_read_rows_misses_the_no_permission_default(dr, uni):
    io = dr.InitializerOption(
        initializer=lambda shape: (torch.arange(shape[0] * shape[1]).reshape(shape) % 7) * 0.5,
        default_value_dim=16, default_value_no_permission=-3.5)
    opt = dr.GradientDescentOptimizer(L.LR)
    a, b = make(dr, True, init_option=io), make(dr, False, init_option=io)
    ks = uni.keys[:160]
    for ev in (a, b):
        train(dr, opt, ev, ks, 0)
    assert a.demote_to(40) == 120
    tk = tier_state(a)[0]
    ids = np.concatenate([tk[:40], NEVER[:24]])
    for sp in (onehot_sp(dr, ids),
               bag_sp(dr, np.random.default_rng(7), lambda n: np.resize(ids, n))[0]):
        out = serve_both(dr, [a], [b], lambda evs: dr.embedding_lookup_sparse(
            evs[0], sp, combiner="sum"))
    o = bits(serve_both(dr, [a], [b], lambda evs: dr.embedding_lookup_sparse(
        evs[0], onehot_sp(dr, ids), combiner="sum")))
    miss = np.full((1, 8), -3.5, np.float32).view(np.int32)
    assert (o[40:] == miss).all() and (o[:40] != miss).any()
    assert out is not None


# ---------------------------------------------------------------------------
# 4. nothing extra runs where it should not; what stays refused
# ---------------------------------------------------------------------------
def test_no_extra_launches(dr, uni, monkeypatch):
    opt = dr.GradientDescentOptimizer(L.LR)
    a, b = make(dr, True), make(dr, False)
    ks = uni.keys[:200]
    for ev in (a, b):
        train(dr, opt, ev, ks, 0)
    lib = dr._lib.lib()
    calls = []
    for name in ("dr_ev_missing_keys", "dr_ev_overlay_resolve", "dr_ev_overlay_patch_onehot"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: calls.append(_n) or _r(*a))
    rng = np.random.default_rng(9)
    sp1 = onehot_sp(dr, ks[:B])
    spb, _ = bag_sp(dr, rng, lambda n: rng.choice(ks, n))

    def both(evs):
        return torch.cat([dr.embedding_lookup_sparse(evs[0], sp1, combiner="sum"),
                          dr.embedding_lookup_sparse(evs[0], spb, combiner="sum")], 1)
    assert a.tier_count() == 0
    serve_both(dr, [a], [b], both)
    assert calls == []                          # an empty tier: no launch, opted in or not
    with dr.read_only_lookups():
        both([a])
    assert calls == []
    assert a.demote_to(60) == 140
    res = a.export()[0].cpu().numpy()
    res = res[~np.isin(res, tier_state(a)[0])]
    assert res.size == 60
    sp1 = onehot_sp(dr, np.resize(res, B))
    spb, _ = bag_sp(dr, rng, lambda n: rng.choice(res, n))
    serve_both(dr, [a], [b], both)
    # resident keys only: one missing-keys launch per lookup, no overlay launch
    assert calls == ["dr_ev_missing_keys"] * 2, calls


def test_what_stays_refused(dr, pooled):
    As, Bs, tks, hks = pooled
    a = As[0]
    sp = onehot_sp(dr, tks[0][:B])
    s0, t0 = snap(a), tier_state(a)
    for ctx in (dr.read_only_lookups(), dr.read_only_lookups(serve_tier=False)):
        with ctx:
            with pytest.raises(dr.InvalidArgumentError, match=r"promote\(keys\) first"):
                dr.embedding_lookup_sparse(a, sp, combiner="sum")
            with pytest.raises(dr.InvalidArgumentError, match=r"promote\(keys\) first"):
                dr.embedding_lookup_sparse_multi([a, a], [sp, sp], combiner="sum")
    # under stream capture with a non-empty tier: refused, opted in or not
    g = torch.cuda.CUDAGraph()
    x, errs = torch.zeros(8, device=DEV), []
    rng = np.random.default_rng(2)
    spb, _ = bag_sp(dr, rng, lambda n: rng.choice(tks[0], n))
    with torch.cuda.graph(g):
        x += 1
        for s in (sp, spb):
            try:
                with dr.read_only_lookups(serve_tier=True):
                    dr.embedding_lookup_sparse(a, s, combiner="sum")
                errs.append(None)
            except dr.InvalidArgumentError as e:
                errs.append(e)
    assert all(e is not None and "cannot be captured" in str(e) for e in errs), errs
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    assert not dr.read_only_serves_tier()
    same(snap(a), s0, "export() after the refusals")
    same(tier_state(a), t0, "the host tier after the refusals")
    dr.status_check()


# ---------------------------------------------------------------------------
# 5. the two kernels alone, through ctypes
# ---------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _overlay(rng, sizes):
    """Per-table sorted distinct keys (the special ones included where there
    is room), concatenated, and the host prefix."""
    parts, off = [], [0]
    for n in sizes:
        k = rng.choice(np.arange(-3000, 3000, dtype=np.int64), n, replace=False) if n else \
            np.empty(0, np.int64)
        if n >= 8:
            k[:4] = SPECIAL
        parts.append(np.unique(k))
        assert parts[-1].size == n
        off.append(off[-1] + n)
    return parts, np.concatenate(parts), off


@pytest.mark.parametrize("sizes", [(0, 0, 1), (1, 0, 0), (600, 0, 400)],
                         ids=["M1-last", "M1-first", "M1000"])
def test_overlay_resolve_against_searchsorted(dr, sizes):
    rng = np.random.default_rng(sum(sizes))
    parts, ov, off = _overlay(rng, sizes)
    n = [700, 300, 520]
    koff = np.concatenate([[0], np.cumsum(n)])
    keys = rng.integers(-3100, 3100, koff[-1]).astype(np.int64)
    for t in range(3):      # every overlay key asked for at least once, the special ones too
        m = min(parts[t].size, n[t] // 2)
        keys[koff[t]:koff[t] + m] = rng.permutation(parts[t])[:m]
    keys[koff[1] - 4:koff[1]] = SPECIAL
    rows = rng.integers(0, 1000, koff[-1]).astype(np.int64)
    neg = rng.random(koff[-1]) < 0.6
    for t in range(3):
        neg[koff[t]:koff[t] + min(parts[t].size, 3)] = True     # (hits, however small M is)
    rows[neg] = -(np.arange(koff[-1]) - koff[np.searchsorted(koff[1:], np.arange(koff[-1]),
                                                             side="right")] + 1)[neg]
    n_dev = [T(np.array([450], np.int64)), None, T(np.array([n[2]], np.int64))]   # table 0 cut
    want = rows.copy()
    for t in range(3):
        cut = 450 if t == 0 else n[t]
        for i in range(koff[t], koff[t] + cut):
            if rows[i] < 0:
                j = np.searchsorted(parts[t], keys[i])
                hit = j < parts[t].size and parts[t][j] == keys[i]
                want[i] = -(2 + off[t] + j) if hit else -1
    dk, dov, drows = T(keys), T(ov), T(rows)
    rc = dr._lib.lib().dr_ev_overlay_resolve(
        dk.data_ptr(), (C.c_int64 * 4)(*koff.tolist()),
        (C.c_void_p * 3)(*[None if x is None else x.data_ptr() for x in n_dev]), 3,
        dov.data_ptr(), (C.c_int64 * 4)(*off), drows.data_ptr(), _stream())
    assert rc == 0
    got = drows.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[rows >= 0], rows[rows >= 0])      # untouched
    np.testing.assert_array_equal(got[450:700], rows[450:700])           # past the device count
    live = np.ones(koff[-1], bool)
    live[450:700] = False
    changed = got[(rows < 0) & live]
    assert ((changed == -1) | ((changed <= -2) & (changed >= -(1 + ov.size)))).all()
    assert (changed <= -2).sum() >= 1
    dr.status_check()


PATCH = [("float32", 4, 0, False), ("float32", 128, 0, False), ("float32", 256, 1, False),
         ("float32", 16, 1, False), ("bfloat16", 8, 0, False), ("bfloat16", 64, 0, True)]


@pytest.mark.parametrize("dtype,dim,order,out_bf16", PATCH)
def test_overlay_patch_against_a_scatter(dr, dtype, dim, order, out_bf16):
    rng = np.random.default_rng(dim + order)
    Tn = 3
    parts, ov, off = _overlay(rng, (40, 0, 25))
    M = off[-1]
    vals = rng.integers(-8, 9, (M, dim)).astype(np.float32) * 0.5
    vals[vals == 0] = -0.0                   # the SEQ order turns -0.0 into +0.0
    rows = torch.as_tensor(vals).to(TORCH_DT[dtype])
    odt = torch.bfloat16 if out_bf16 else torch.float32
    out0 = torch.full((B, Tn * dim + 8), 7.0, dtype=odt)
    stride = Tn * dim + 8
    # the miss list: positions t * B + b with their keys; hits, keys the overlay lacks, a
    # table with an empty range, duplicates, and two positions out of range
    pos = rng.permutation(Tn * B)[:120]
    key = np.empty(pos.size, np.int64)
    for i, p in enumerate(pos):
        t = p // B
        key[i] = rng.choice(parts[t]) if parts[t].size and rng.random() < 0.7 else 5000 + i
    pos = np.concatenate([pos, pos[:30], [-1, Tn * B]])
    key = np.concatenate([key, key[:30], [parts[0][0], parts[0][0]]])
    want = out0.clone()
    hits = 0
    for p, k in zip(pos.tolist(), key.tolist()):
        if not 0 <= p < Tn * B:
            continue
        t, b = divmod(p, B)
        j = np.searchsorted(parts[t], k)
        if j < parts[t].size and parts[t][j] == k:
            r = rows[off[t] + j]
            r = r.to(odt) if odt == torch.bfloat16 else r.float()
            if order == 1:
                r = 0.0 + r
            want[b, t * dim:(t + 1) * dim] = r
            hits += 1
    assert hits > 40
    dk, dp, dov = T(key), T(pos.astype(np.int64)), T(ov)
    drows, out = rows.to(DEV).contiguous(), out0.to(DEV)
    words = dim // 2 if dtype == "bfloat16" else dim
    koff = (C.c_int64 * 4)(0, B, 2 * B, 3 * B)
    rc = dr._lib.lib().dr_ev_overlay_patch_onehot(
        dk.data_ptr(), dp.data_ptr(), key.size, koff, Tn, dov.data_ptr(), (C.c_int64 * 4)(*off),
        drows.data_ptr(), words, out.data_ptr(), stride, dim, order,
        dr._lib.LOOKUP_OUT_BF16 if out_bf16 else 0, _stream())
    assert rc == 0, dr._lib.lib().dr_last_error()
    np.testing.assert_array_equal(bits(out), bits(want))
    if order == 1:
        assert not (bits(out) == np.int32(-2 ** 31)).any()       # no -0.0 left
    else:
        assert (bits(out.float()) == np.int32(-2 ** 31)).any()    # ALI: a bitwise copy
    dr.status_check()


# ---------------------------------------------------------------------------
# 6. the serving walk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS)
def test_serving_walk_equals_twin(dr, seed):
    ops, counts = S.walk(seed)
    a, b = make(dr, True, filter_freq=S.FILTER_FREQ), make(dr, False, filter_freq=S.FILTER_FREQ)
    opt = dr.GradientDescentOptimizer(L.LR)
    served = 0
    for op in ops:
        if op["op"] == "train":
            for ev in (a, b):
                train(dr, opt, ev, op["keys"], op["step"], seed=seed)
        elif op["op"] == "sight":
            for ev in (a, b):
                ev.sparse_read(T(op["keys"]))
        elif op["op"] == "demote":
            n = int(a.total_count()[0])
            assert a.demote_to(0) == n and int(a.total_count()[0]) == 0
        elif op["op"] == "end":
            np.testing.assert_array_equal(tier_state(a)[0], op["tier"])
        else:
            sp = dr.SparseTensor(T(op["indices"]), T(op["values"]),
                                 (S.BAGS, op["width"]))
            out = serve_both(dr, [a], [b], lambda evs: dr.embedding_lookup_sparse(
                evs[0], sp, combiner=op["combiner"]))
            tk = tier_state(a)[0]
            # the model's places are the EV's
            cls = op["classes"]
            in_tier = np.isin(op["values"], tk)
            np.testing.assert_array_equal(
                in_tier, (cls == S.SERVED) | (cls == S.FILTERED) | (cls == S.OTHER))
            served += int((cls == S.SERVED).sum())
            if op["kind"] == "onehot":
                o, d = bits(out), default_bits(a)
                assert (o[(cls == S.FILTERED) | (cls == S.NEVER)] == d).all()
                assert (o[cls == S.SERVED] != d).any()
    assert served == counts[S.SERVED] >= 200
    same(snap(a), snap(b), "the merged export at the end of the walk")
    dr.status_check()
