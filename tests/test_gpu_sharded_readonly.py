"""Read-only forward of the sharded lookup engines (evaluation and serving).

The reference everywhere is code that predates these engines' read-only
forward: dr_ev_gather_readonly per table, or read_only_lookups() +
embedding_lookup_sparse_multi on full local twin tables holding the same
rows.  Every comparison is bit-exact (bits()), and every table's snapshot
(export + key_meta + total_count) is taken before and after and must be
equal.  Tables hold keys 0 .. N_KEYS-1; ids are drawn from [0, ID_SPACE), so
about a third are absent.  Every shard's default row is the same constant as
the twin's: the engines serve the OWNER's default row.

Multi-rank cases run the ranks as threads (worlds 1-3) with bounded barriers
and joins, or as processes driven by tools/sharded_readonly_check.py."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_KEYS, ID_SPACE = 100, 150
DEFAULT = 0.5
WAIT = 60          # seconds: barrier / join bound of the threaded ranks


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd
    deeprec_amd.load()
    deeprec_amd.set_validate(True)
    assert torch.cuda.is_available()
    return deeprec_amd


def T_(x, dtype=None):
    return torch.as_tensor(np.asarray(x), device=DEV, dtype=dtype)


def H(t):
    return t.detach().cpu().numpy()


def bits(t):
    """A tensor's bytes (bit-equality of any dtype, bf16 and -0.0 included)."""
    return H(t.detach().contiguous().reshape(-1).view(torch.uint8))


def snapshot(ev, probe=None):
    probe = np.arange(ID_SPACE, dtype=np.int64) if probe is None else probe
    k, v, ver, fr = ev.export()
    f, vv, hr = ev.key_meta(np.asarray(probe, np.int64))
    return [np.asarray(int(ev.total_count()[0])), H(k), bits(v), H(ver), H(fr), f, vv, hr]


def assert_same_state(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _rows(t, keys, D):
    k = np.asarray(keys, np.float64)[:, None]
    r = np.cos(0.013 * k + 0.7 * t + 0.05 * np.arange(D)[None, :]).astype(np.float32)
    r[np.asarray(keys) % 5 == 0, 0] = -0.0      # by key: a shard and the twin hold the same rows
    return r


def _handles(evs):
    return (C.c_void_p * len(evs))(*[e.handle.value for e in evs])


def _run_ranks(world, fn, bar=None):
    """fn(rank) on `world` threads; the first failure aborts the barrier so
    no rank stays in it, and joins are bounded."""
    errs = []

    def run(r):
        try:
            fn(r)
        except BaseException as e:  # noqa: BLE001 -- surfaced below
            errs.append(e)
            if bar is not None:
                bar.abort()

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for x in th:
        x.start()
    for x in th:
        x.join(WAIT)
    if errs:
        raise errs[0]
    assert not any(x.is_alive() for x in th), "a rank did not finish"


# ---------------------------------------------------------------------------
# 1. the tagged entry, one process
# ---------------------------------------------------------------------------
def _gather_ro(ev, keys):
    """The reference: dr_ev_gather_readonly of one table."""
    from deeprec_amd._lib import check, lib, ptr, stream_handle
    n = int(keys.numel())
    out = torch.empty((n, ev.dim), dtype=ev.value_dtype, device=DEV)
    check(lib().dr_ev_gather_readonly(ev.handle, ptr(keys), n, None, ptr(out), stream_handle(DEV)))
    return out


def _tagged_ro(evs, keys, tags, n, n_dev, out):
    from deeprec_amd._lib import check, lib, ptr, stream_handle
    check(lib().dr_ev_gather_tagged_readonly(_handles(evs), len(evs), ptr(keys), ptr(tags), n,
                                             ptr(n_dev), ptr(out), stream_handle(DEV)))


@pytest.mark.parametrize("D,vdt,slot", [(4, torch.float32, True), (6, torch.float32, False),
                                        (12, torch.float32, True), (64, torch.float32, False),
                                        (256, torch.float32, False), (16, torch.bfloat16, False)])
def test_tagged_entry(dr, D, vdt, slot):
    name = "srt_%d_%s" % (D, "b" if vdt == torch.bfloat16 else "f")
    allk = np.arange(N_KEYS, dtype=np.int64)
    # table 0: grown past its initial capacity (64 -> 100 keys)
    ev0 = dr.EmbeddingVariable(name + "_0", D, DEFAULT, capacity=64, value_dtype=vdt)
    ev0.insert(T_(allk), T_(_rows(0, allk, D)).to(vdt))
    # table 1: Counter EV; keys 0..59 admitted, 60..99 bulk-inserted rows that
    # exist below the threshold (freq 0): their default is served
    ev1 = dr.EmbeddingVariable(name + "_1", D, DEFAULT * 2, capacity=256, value_dtype=vdt,
                               ev_option=dr.EmbeddingVariableOption(
                                   filter_option=dr.CounterFilter(3)))
    ev1.insert(T_(allk[:60]), T_(_rows(1, allk[:60], D)).to(vdt))
    ev1.insert_synthetic(60, 40, seed=5)
    f1, _, hr1 = ev1.key_meta(allk)
    np.testing.assert_array_equal(hr1, [True] * 100)
    np.testing.assert_array_equal(f1, [3] * 60 + [0] * 40)
    # table 2: a slot column whose first-touch bit is set for keys 0..29 only
    # (slot default served elsewhere), or a plain table
    ev2 = dr.EmbeddingVariable(name + "_2", D, DEFAULT * 3, capacity=256, value_dtype=vdt)
    ev2.insert(T_(allk), T_(_rows(2, allk, D)).to(vdt))
    t2 = ev2
    if slot:
        t2 = ev2.slot("Adagrad", 0.1)
        g = np.random.default_rng(3).standard_normal((30, D)).astype(np.float32)
        ev2.pending_grads.append(dr.IndexedSlices(T_(g), T_(allk[:30])))
        dr.AdagradOptimizer(np.float32(0.1), 0.1).apply_gradients([ev2], global_step=0)
        np.testing.assert_array_equal(t2.key_meta(allk)[2], allk < 30)
    tables = [ev0, ev1, t2]
    prim = [ev0, ev1, ev2]
    s0 = [snapshot(e) for e in prim] + [t2.key_meta(np.arange(ID_SPACE))[2]]
    rng = np.random.default_rng(100 + D)
    for n in (1, 5, 67):
        keys = rng.integers(0, ID_SPACE, n).astype(np.int64)
        tags = ((np.arange(n) + n) % 3).astype(np.int32)            # interleaved
        kt, tt = T_(keys), T_(tags)
        refs = [_gather_ro(e, kt) for e in tables]                   # [n, D] per table
        want = torch.stack(refs)[tt.long(), torch.arange(n, device=DEV)]
        out = torch.full((n, D), 7.0, dtype=vdt, device=DEV)
        _tagged_ro(tables, kt, tt, n, None, out)
        np.testing.assert_array_equal(bits(out), bits(want))
        if n == 67:
            # every serving rule is in the batch
            served = [H(e.find(kt)) >= 0 for e in tables]
            assert (keys >= N_KEYS).sum() > 10
            assert ((tags == 1) & (keys >= 60) & (keys < N_KEYS)).any() and not \
                served[1][(keys >= 60)].any()
            if slot:
                assert ((tags == 2) & (keys >= 30) & (keys < N_KEYS)).any()
                sel = (tags == 2) & (keys >= 30)
                assert (H(out.float())[sel] == np.float32(0.1)).all()
        # n_dev < n: the tail of a sentinel-filled out is untouched
        if n > 1:
            m = n // 2
            out2 = torch.full((n, D), 7.0, dtype=vdt, device=DEV)
            _tagged_ro(tables, kt, tt, n, T_(np.array([m], np.int64)), out2)
            np.testing.assert_array_equal(bits(out2[:m]), bits(want[:m]))
            np.testing.assert_array_equal(bits(out2[m:]),
                                          bits(torch.full((n - m, D), 7.0, dtype=vdt, device=DEV)))
    _tagged_ro(tables, None, None, 0, None, None)                    # n == 0: OK
    dr.status_check()
    s1 = [snapshot(e) for e in prim] + [t2.key_meta(np.arange(ID_SPACE))[2]]
    for a, b in zip(s0[:3], s1[:3]):
        assert_same_state(a, b)
    np.testing.assert_array_equal(s0[3], s1[3])


# ---------------------------------------------------------------------------
# 2. ShardedLookup, ranks as threads
# ---------------------------------------------------------------------------
ST, SB, SD = 3, 37, 16


class _Exchange(object):
    """all_to_all_single between threads of one process."""

    def __init__(self, world):
        self.world = world
        self.bar = threading.Barrier(world, timeout=WAIT)
        self.box = [None] * world

    def a2a(self, rank, out, inp, out_splits, in_splits):
        W = self.world
        if in_splits is None:
            in_splits = [inp.shape[0] // W] * W
        if out_splits is None:
            out_splits = [out.shape[0] // W] * W
        self.box[rank] = list(torch.split(inp, list(in_splits)))
        self.bar.wait()
        pieces = [self.box[p][rank] for p in range(W)]
        assert [x.shape[0] for x in pieces] == list(out_splits)
        if out.shape[0]:
            torch.cat(pieces, out=out)
        self.bar.wait()
        return out


def _make_tables(dr, tag, keys, D, vdt=torch.float32, counter=True, nT=ST):
    """nT tables over `keys` (a shard's or all): 0 plain and grown past its
    capacity when it holds all keys, 1 a Counter EV (keys < 80 admitted, the
    others bulk-inserted below the threshold) unless counter=False, 2 plain."""
    keys = np.asarray(keys, np.int64)
    evs = []
    for t in range(nT):
        if t == 1 and counter:
            ev = dr.EmbeddingVariable("%s_%d" % (tag, t), D, DEFAULT, capacity=256,
                                      value_dtype=vdt, device=DEV,
                                      ev_option=dr.EmbeddingVariableOption(
                                          filter_option=dr.CounterFilter(3)))
            adm, low = keys[keys < 80], keys[keys >= 80]
            ev.insert(T_(adm), T_(_rows(t, adm, D)).to(vdt))
            if low.size:     # a shard's keys are an arithmetic progression
                stride = int(low[1] - low[0]) if low.size > 1 else 1
                ev.insert_synthetic(int(low[0]), int(low.size), seed=9, key_stride=stride)
        else:
            ev = dr.EmbeddingVariable("%s_%d" % (tag, t), D, DEFAULT, capacity=64,
                                      value_dtype=vdt, device=DEV)
            ev.insert(T_(keys), T_(_rows(t, keys, D)).to(vdt))
        evs.append(ev)
    return evs


def _twin_ref(dr, full, ids, off, combiner, out_dtype=None):
    """read_only_lookups() + embedding_lookup_sparse_multi on the full twins."""
    from deeprec_amd.embedding_ops import SparseTensor, embedding_lookup_sparse_multi
    bags = off.shape[0] - 1
    seg = np.repeat(np.arange(bags), np.diff(off))
    ind = T_(np.stack([seg, np.zeros_like(seg)], 1).astype(np.int64))
    width = max(1, int(np.diff(off).max()))
    sps = [SparseTensor(ind, T_(ids[t]), (bags, width)) for t in range(len(full))]
    kw = {} if out_dtype is None else {"out_dtype": out_dtype}
    with torch.no_grad(), dr.read_only_lookups():
        return embedding_lookup_sparse_multi(full, sps, combiner=combiner, **kw)


def _bag_batch(rng, nT, bags, max_nnz=None):
    lens = rng.integers(0, 4, bags)
    lens[0], lens[3] = 3, 0
    if max_nnz is not None:
        while lens.sum() > max_nnz:
            lens[int(np.argmax(lens))] -= 1
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.integers(0, ID_SPACE, (nT, int(off[-1]))).astype(np.int64)
    ids[:, :3] = 11
    return ids, off


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharded_lookup_read_only(dr, world):
    from deeprec_amd.sharded import ShardedLookup
    allk = np.arange(N_KEYS, dtype=np.int64)
    full = _make_tables(dr, "srl%d_full" % world, allk, SD)
    ex = _Exchange(world)
    engines = []
    for r in range(world):
        evs = _make_tables(dr, "srl%d_r%d" % (world, r), allk[allk % world == r], SD)
        eng = ShardedLookup(evs, world, r, SB, torch.device(DEV))
        eng._a2a = (lambda rr: (lambda out, inp, os_=None, is_=None:
                                ex.a2a(rr, out, inp, os_, is_)))(r)
        engines.append(eng)
    assert engines[0].backend.filter                     # table 1 counts sightings in training
    s0 = [[snapshot(e) for e in eng.evs] for eng in engines]
    f0 = [snapshot(e) for e in full]
    rng = np.random.default_rng(50 + world)
    onehot_off = np.arange(SB + 1, dtype=np.int32)
    cases = []
    for name in ("onehot", "onehot_mod3", "sum", "mean"):
        per_rank = []
        for r in range(world):
            if name.startswith("onehot"):
                ids = rng.integers(0, ID_SPACE, (ST, SB)).astype(np.int64)
                ids[:, :4] = 11
                if name == "onehot_mod3":                # world 3: two owners receive nothing
                    ids = ids // 3 * 3
                per_rank.append((ids, onehot_off))
            else:
                per_rank.append(_bag_batch(rng, ST, SB))
        cases.append((name, "sum" if name.startswith("onehot") else name, per_rank))
    for name, combiner, per_rank in cases:
        onehot = name.startswith("onehot")
        refs = [_twin_ref(dr, full, ids, off, combiner) for ids, off in per_rank]
        for mode in ("argument", "context"):
            outs = [None] * world

            def rank(r):
                ids, off = per_rank[r]
                bo = None if onehot else [T_(off)] * ST
                with torch.no_grad():
                    if mode == "argument":
                        o = engines[r].forward(T_(ids), bag_offs=bo, combiner=combiner,
                                               read_only=True)
                    else:                                # the context is per thread
                        with dr.read_only_lookups():
                            o = engines[r].forward(T_(ids), bag_offs=bo, combiner=combiner)
                outs[r] = o.clone()

            _run_ranks(world, rank, ex.bar)
            dr.status_check()
            for r in range(world):
                np.testing.assert_array_equal(bits(outs[r]), bits(refs[r]), err_msg="%s %s rank %d"
                                              % (name, mode, r))
                st = engines[r].last_stats
                # one-hot routes directly although table 1 filters: no Unique
                assert st["direct"] == onehot and engines[r]._saved is None
                if world > 1:
                    assert st["read_only"] is True
                with pytest.raises(RuntimeError):
                    engines[r].backward(torch.zeros(SB, ST * SD, device=DEV))
    with pytest.raises(ValueError):
        engines[0].forward(T_(cases[0][2][0][0]), need_grad=True, read_only=True)
    for r in range(world):
        for a, e in zip(s0[r], engines[r].evs):
            assert_same_state(a, snapshot(e))
            assert not e.pending_grads
    for a, e in zip(f0, full):
        assert_same_state(a, snapshot(e))


# ---------------------------------------------------------------------------
# 3. XgmiShardedLookup, ranks as threads
# ---------------------------------------------------------------------------
def _xgmi_engines(dr, tag, world, vdt, dedup):
    from deeprec_amd.sharded import XgmiBuffers, XgmiShardedLookup
    allk = np.arange(N_KEYS, dtype=np.int64)
    evs_all = [_make_tables(dr, "%s_r%d" % (tag, r), allk[allk % world == r], SD, vdt,
                            counter=False) for r in range(world)]
    bufs = [XgmiBuffers(world, ST, SB, SD, DEV, value_dtype=vdt)
            for _ in range(world)]
    bar = threading.Barrier(world, timeout=WAIT)
    engines = [XgmiShardedLookup(evs_all[r], world, r, SB, torch.device(DEV), peer_buffers=bufs,
                                 barrier=bar.wait, buffers=bufs[r], dedup=dedup)
               for r in range(world)]
    return engines, bar


def _xgmi_forward(dr, engines, bar, per_rank, combiner="sum", bags=False, out_dtype=None,
                  context=False, read_only=True):
    world = len(engines)
    outs = [None] * world

    def rank(r):
        ids, off = per_rank[r]
        kw = {"out_dtype": out_dtype}
        if bags:
            kw.update(bag_offs=[T_(off)] * ST, combiner=combiner)
        if context:
            with dr.read_only_lookups():
                o = engines[r].forward(T_(ids), **kw)
        else:
            o = engines[r].forward(T_(ids), read_only=read_only, **kw)
        bar.wait()                                   # every owner has written every output
        outs[r] = o.clone()
        bar.wait()                                   # ... and it is copied before the next route

    _run_ranks(world, rank, bar)
    dr.status_check()
    return outs


@pytest.mark.parametrize("world", [1, 2, 3])
def test_xgmi_read_only(dr, world):
    allk = np.arange(N_KEYS, dtype=np.int64)
    full = _make_tables(dr, "sxr%d_full" % world, allk, SD, counter=False)
    plain, bar_p = _xgmi_engines(dr, "sxr%d_p" % world, world, torch.float32, False)
    dedup, bar_d = _xgmi_engines(dr, "sxr%d_d" % world, world, torch.float32, True)
    rng = np.random.default_rng(60 + world)
    off1 = np.arange(SB + 1, dtype=np.int32)

    def onehot_batch():
        out = []
        for r in range(world):
            ids = rng.integers(0, ID_SPACE, (ST, SB)).astype(np.int64)
            ids[:, :4] = 13
            out.append((ids, off1))
        return out

    s_p = [[snapshot(e) for e in eng.evs] for eng in plain]
    s_d = [[snapshot(e) for e in eng.evs] for eng in dedup]
    # plain one-hot: the argument, then the context
    for context in (False, True):
        batch = onehot_batch()
        outs = _xgmi_forward(dr, plain, bar_p, batch, context=context)
        for r in range(world):
            np.testing.assert_array_equal(bits(outs[r]),
                                          bits(_twin_ref(dr, full, *batch[r], "sum")))
            assert plain[r]._saved is None
            # the plain path keeps no state in training: after a read-only
            # forward its backward must refuse all the same
            with pytest.raises(RuntimeError):
                plain[r].backward(torch.zeros(SB, ST * SD, device=DEV))
    # per-destination dedup
    batch = onehot_batch()
    outs = _xgmi_forward(dr, dedup, bar_d, batch)
    for r in range(world):
        np.testing.assert_array_equal(bits(outs[r]), bits(_twin_ref(dr, full, *batch[r], "sum")))
        assert dedup[r]._saved is None
        with pytest.raises(RuntimeError):
            dedup[r].backward(torch.zeros(SB, ST * SD, device=DEV))
    # multi-hot bags, mean (nnz <= the engine's per-table capacity)
    bagb = [_bag_batch(rng, ST, SB, max_nnz=SB) for _ in range(world)]
    outs = _xgmi_forward(dr, plain, bar_p, bagb, combiner="mean", bags=True)
    for r in range(world):
        np.testing.assert_array_equal(bits(outs[r]), bits(_twin_ref(dr, full, *bagb[r], "mean")))
        assert plain[r]._saved is None
        with pytest.raises(RuntimeError):
            plain[r].backward(torch.zeros(SB, ST * SD, device=DEV))
    # no table of any rank -- owner or requester -- has changed
    for engs, snaps in ((plain, s_p), (dedup, s_d)):
        for r in range(world):
            for a, e in zip(snaps[r], engs[r].evs):
                assert_same_state(a, snapshot(e))
                assert not e.pending_grads
    # a following training forward still inserts the absent keys, at their owners
    batch = onehot_batch()
    outs = _xgmi_forward(dr, plain, bar_p, batch, read_only=False)
    for r in range(world):
        np.testing.assert_array_equal(bits(outs[r]), bits(_twin_ref(dr, full, *batch[r], "sum")))
        for t in range(ST):
            asked = np.unique(np.concatenate([b[0][t] for b in batch]))
            new = asked[(asked >= N_KEYS) & (asked % world == r)]
            assert new.size > 0
            k = H(plain[r].evs[t].export()[0])
            assert np.isin(new, k).all() and k.size == (allk % world == r).sum() + new.size
    # ... after which the backward works again
    grads = torch.zeros(SB, ST * SD, device=DEV)
    _run_ranks(world, lambda r: plain[r].backward(grads), bar_p)
    for eng in plain:
        for e in eng.evs:
            e.pending_grads.clear()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_xgmi_read_only_bf16(dr, world):
    allk = np.arange(N_KEYS, dtype=np.int64)
    full = _make_tables(dr, "sxb%d_full" % world, allk, SD, torch.bfloat16, counter=False)
    engines, bar = _xgmi_engines(dr, "sxb%d" % world, world, torch.bfloat16, False)
    s0 = [[snapshot(e) for e in eng.evs] for eng in engines]
    rng = np.random.default_rng(70 + world)
    off1 = np.arange(SB + 1, dtype=np.int32)
    batch = [(rng.integers(0, ID_SPACE, (ST, SB)).astype(np.int64), off1) for _ in range(world)]
    for od in (None, torch.bfloat16):
        outs = _xgmi_forward(dr, engines, bar, batch, out_dtype=od)
        for r in range(world):
            ref = _twin_ref(dr, full, *batch[r], "sum", out_dtype=od)
            assert outs[r].dtype == (od or torch.float32) == ref.dtype
            np.testing.assert_array_equal(bits(outs[r]), bits(ref))
    for r in range(world):
        for a, e in zip(s0[r], engines[r].evs):
            assert_same_state(a, snapshot(e))


# ---------------------------------------------------------------------------
# 4. the native engine, world 2, separate processes
# ---------------------------------------------------------------------------
def test_native_engines_read_only_multiprocess():
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sharded_readonly_check.py"),
                        "--world", "2", "--timeout", "100"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=150)
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-4000:]
    assert sorted(x["rank"] for x in lines) == [0, 1]
    bad = [(x["rank"], c[0]) for x in lines for c in x["checks"] if not c[1]]
    assert not bad, bad
    assert all(x["ok"] for x in lines)
    names = {c[0] for c in lines[0]["checks"]}
    for kind in ("rccl", "fixed", "xgmi"):
        assert {"%s_onehot" % kind, "%s_onehot_context" % kind, "%s_backward_refuses" % kind,
                "%s_need_grad_refused" % kind, "%s_shards_unchanged" % kind} <= names
    for kind in ("rccl", "fixed"):
        assert {"%s_bags_mean" % kind, "%s_bf16_fp32" % kind, "%s_bf16_bf16" % kind} <= names


# ---------------------------------------------------------------------------
# 5. model zoo
# ---------------------------------------------------------------------------
def test_dlrm_sharded_eval_leaves_the_tables_alone(dr):
    from deeprec_amd import modelzoo as mz
    from deeprec_amd.sharded import XgmiShardedLookup
    torch.manual_seed(7)
    nT, R, D, B = 2, 50, 16, 32
    rows = [torch.randn(R, D, device=DEV) * 0.1 for _ in range(nT)]

    def tables(tag):
        evs = []
        for t in range(nT):
            ev = dr.EmbeddingVariable("srm_%s_%d" % (tag, t), D, 0.0, device=DEV)
            ev.insert(torch.arange(R, device=DEV), rows[t])
            evs.append(ev)
        return evs

    evs_s, evs_l = tables("s"), tables("l")
    eng = XgmiShardedLookup(evs_s, 1, 0, B, torch.device(DEV))
    sharded = mz.DLRM(evs_s, 13, (32,), (32, 16), engine=eng).to(DEV)
    local = mz.DLRM(evs_l, 13, (32,), (32, 16)).to(DEV)
    local.load_state_dict(sharded.state_dict())
    dense = torch.randn(B, 13, device=DEV)
    ids = torch.randint(0, R, (nT, B), device=DEV)
    ids[:, ::2] = torch.randint(1000, 2000, (nT, B // 2), device=DEV)      # unseen
    with dr.read_only_lookups():
        p = sharded(dense, ids)
        q = local(dense, ids)
    assert [int(ev.total_count()[0]) for ev in evs_s] == [R, R]
    assert not any(ev.pending_grads for ev in evs_s)
    np.testing.assert_array_equal(bits(p), bits(q))
    p.sum().backward()                                   # the dense part still trains
    assert sharded.last.weight.grad is not None
    assert not any(ev.pending_grads for ev in evs_s)
    with torch.no_grad():
        sharded(dense, ids)                              # outside: insert-on-miss
    assert all(int(ev.total_count()[0]) > R for ev in evs_s)
    dr.status_check()
