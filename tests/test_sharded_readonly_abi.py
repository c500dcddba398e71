"""CPU-side checks of the sharded engines' read-only forward: the two C
entries (dr_ev_gather_tagged_readonly, dr_xgmi_serve_readonly) and the
DR_SHARDED_READ_ONLY flag resolve and refuse null arguments before they touch
a device, and ShardedLookup's read-only protocol runs over a world-2 gloo
group with a dict backend: one-hot ids route directly even for a filter
backend, the owner serves through find_pack (never resolve_pack), an absent
key gets the OWNER's default row, and no backward state is kept."""
import ctypes as C
import datetime
import os
import re
import socket
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
HEADER = os.path.join(ROOT, "include", "deeprec_amd.h")
INVALID_ARGUMENT = 3
ENTRIES = ("dr_ev_gather_tagged_readonly", "dr_xgmi_serve_readonly")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "deeprec-1_amd")])
    import deeprec_amd._lib as L
    lib = C.CDLL(LIB)
    for name in ENTRIES + ("dr_sharded_forward", "dr_last_error", "dr_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def test_entries_resolve_and_abi_version_stays(lib):
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.dr_abi_version() == 2


def test_mirror_binds_the_entries_and_the_flag():
    import deeprec_amd._lib as L
    for name in ENTRIES:
        assert name in L.SIGNATURES, name
    assert L.SHARDED_READ_ONLY == 2
    m = re.search(r"^#define\s+DR_SHARDED_READ_ONLY\s+(\d+)\s*$", open(HEADER).read(), re.M)
    assert m and int(m.group(1)) == L.SHARDED_READ_ONLY
    assert L.SHARDED_READ_ONLY & L.SHARDED_OUT_BF16 == 0
    from deeprec_amd import sharded
    for cls in (sharded.ShardedLookup, sharded.NativeShardedLookup, sharded.XgmiShardedLookup):
        assert cls.supports_read_only is True
    assert not hasattr(sharded.HybridShardedLookup, "supports_read_only") or \
        sharded.HybridShardedLookup.supports_read_only


def test_null_arguments_are_invalid_argument(lib):
    assert lib.dr_ev_gather_tagged_readonly(None, 1, None, None, 4, None, None,
                                            None) == INVALID_ARGUMENT
    assert lib.dr_last_error()
    evs = (C.c_void_p * 2)(None, None)
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    # null keys / tags / out with n > 0, null table entries, a bad table count
    assert lib.dr_ev_gather_tagged_readonly(evs, 2, None, p, 4, None, p, None) == INVALID_ARGUMENT
    assert lib.dr_ev_gather_tagged_readonly(evs, 2, p, None, 4, None, p, None) == INVALID_ARGUMENT
    assert lib.dr_ev_gather_tagged_readonly(evs, 2, p, p, 4, None, None, None) == INVALID_ARGUMENT
    assert lib.dr_ev_gather_tagged_readonly(evs, 2, p, p, 4, None, p, None) == INVALID_ARGUMENT
    assert lib.dr_ev_gather_tagged_readonly(evs, 0, p, p, 4, None, p, None) == INVALID_ARGUMENT
    assert lib.dr_xgmi_serve_readonly(None, None, 1, 4, None) == INVALID_ARGUMENT
    assert lib.dr_xgmi_serve_readonly(None, evs, 2, 4, None) == INVALID_ARGUMENT
    import deeprec_amd._lib as L
    peers = L.DrXgmiPeers()
    peers.world, peers.rank, peers.cap = 1, 0, 8
    assert lib.dr_xgmi_serve_readonly(C.byref(peers), None, 1, 4, None) == INVALID_ARGUMENT
    assert lib.dr_xgmi_serve_readonly(C.byref(peers), evs, 2, 4, None) == INVALID_ARGUMENT
    # the engine entry refuses a null engine whatever the flags
    assert lib.dr_sharded_forward(None, None, None, None, 4, 0, 0, L.SHARDED_READ_ONLY, None,
                                  None) == INVALID_ARGUMENT


# ---------------------------------------------------------------------------
# ShardedLookup's read-only protocol over gloo, dict backend
# ---------------------------------------------------------------------------
T, D, B = 3, 4, 23
N_KEYS, ID_SPACE = 60, 90        # ids in [0, 90): a third absent everywhere


def _row(t, key):
    return (np.float32(100 * t) + np.float32(key) + np.arange(D, dtype=np.float32) / 8)


def _default(owner, t):
    return np.full(D, -1.0 - owner - 10 * t, np.float32)     # differs per owner and table


def _pool(rows, seg, combiner, bags):
    """Position-order fp32 sum (mean) of rows [nnz, D] over bags."""
    out = np.zeros((bags, D), np.float32)
    cnt = np.zeros(bags, np.int64)
    for i in range(rows.shape[0]):
        out[seg[i]] = out[seg[i]] + rows[i]
        cnt[seg[i]] += 1
    if combiner == "mean":
        nz = cnt > 0
        out[nz] = out[nz] / cnt[nz, None].astype(np.float32)
    return out


class DictLocal(object):
    """A filter backend over plain dicts: the four local steps of a read-only
    forward.  resolve_pack (insert-on-miss) must never run."""

    filter = True

    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        self.T, self.dim = T, D
        self.tables = [{k: _row(t, k) for k in range(N_KEYS) if k % world == rank}
                       for t in range(T)]
        self.calls = []

    def unique_grouped(self, vals, koff, counts=None):
        self.calls.append(("unique", counts))
        v = vals.numpy()
        y = np.zeros(v.shape[0], np.int64)
        idx = np.zeros(v.shape[0], np.int32)
        U = []
        for t in range(T):
            seen = {}
            for j, k in enumerate(v[koff[t]:koff[t + 1]]):
                idx[koff[t] + j] = seen.setdefault(int(k), len(seen))
            y[koff[t]:koff[t] + len(seen)] = list(seen)       # first-occurrence order
            U.append(len(seen))
        return torch.from_numpy(y), torch.from_numpy(idx), None, torch.tensor(U)

    def route(self, uniq, koff, U, world):
        u = uniq.numpy()
        items = []
        for t in range(T):
            m = (koff[t + 1] - koff[t]) if U is None else int(U[t])
            items += [(int(u[i]) % world * T + t, i) for i in range(koff[t], koff[t] + m)]
        items.sort(key=lambda x: x[0])                        # stable
        n = u.shape[0]
        keys, tags, perm = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        counts = np.zeros((world, T), np.int64)
        for j, (k, i) in enumerate(items):
            keys[j], tags[j], perm[j] = u[i], k % T, i
            counts[k // T, k % T] += 1
        return (torch.from_numpy(keys), torch.from_numpy(tags), torch.from_numpy(perm),
                torch.from_numpy(counts))

    def resolve_pack(self, keys, tags, n, per_table):
        raise AssertionError("a read-only forward must not resolve with insert-on-miss")

    def find_pack(self, keys, tags, n):
        self.calls.append(("find_pack", n))
        out = np.zeros((n, D), np.float32)
        for i in range(n):
            k, t = int(keys[i]), int(tags[i])
            assert k % self.world == self.rank
            out[i] = self.tables[t].get(k, _default(self.rank, t))
        return torch.from_numpy(out)

    def pool(self, rows_recv, rowsel, idx, koff, bag_offs, batch, combiner):
        rr, rs = rows_recv.numpy(), rowsel.numpy()
        out = np.zeros((batch, T * D), np.float32)
        for t in range(T):
            if idx is None:
                rows = rr[rs[koff[t]:koff[t + 1]]]
            else:
                rows = rr[rs[koff[t] + idx.numpy()[koff[t]:koff[t + 1]].astype(np.int64)]]
            off = np.arange(batch + 1) if bag_offs is None else bag_offs[t].numpy()
            seg = np.repeat(np.arange(batch), np.diff(off))
            out[:, t * D:(t + 1) * D] = _pool(rows, seg, combiner, batch)
        return torch.from_numpy(out)


def _expect(ids, off, combiner, world):
    out = np.zeros((B, T * D), np.float32)
    seg = np.repeat(np.arange(B), np.diff(off))
    for t in range(T):
        rows = np.stack([_row(t, k) if k < N_KEYS else _default(k % world, t) for k in ids[t]])
        out[:, t * D:(t + 1) * D] = _pool(rows, seg, combiner, B)
    return out


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    try:
        import sys
        sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))
        import deeprec_amd as dr
        from deeprec_amd.sharded import ShardedLookup
        be = DictLocal(rank, world)
        before = [dict(tb) for tb in be.tables]
        eng = ShardedLookup(None, world, rank, B, torch.device("cpu"), backend=be)
        rng = np.random.default_rng(40 + rank)
        # one-hot through the argument: direct route although the backend filters
        ids = rng.integers(0, ID_SPACE, (T, B)).astype(np.int64)
        ids[:, :3] = 7
        out = eng.forward(torch.from_numpy(ids), read_only=True).numpy()
        assert eng.last_stats["direct"] is True and eng.last_stats["read_only"] is True
        assert eng._saved is None
        assert [c[0] for c in be.calls] == ["find_pack"]
        np.testing.assert_array_equal(out, _expect(ids, np.arange(B + 1), "sum", world))
        with pytest.raises(RuntimeError):
            eng.backward(torch.zeros(B, T * D))
        with pytest.raises(ValueError):
            eng.forward(torch.from_numpy(ids), need_grad=True, read_only=True)
        # multi-hot mean through the context: Unique kept, without counts
        be.calls.clear()
        lens = rng.integers(0, 4, B)
        lens[0] = 0
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        mids = rng.integers(0, ID_SPACE, (T, int(off[-1]))).astype(np.int64)
        mids[:, :2] = 11
        with dr.read_only_lookups():
            out = eng.forward(torch.from_numpy(mids), bag_offs=[torch.from_numpy(off)] * T,
                              combiner="mean").numpy()
        assert eng.last_stats["direct"] is False and eng.last_stats["read_only"] is True
        assert be.calls[0] == ("unique", False) and be.calls[1][0] == "find_pack"
        assert eng._saved is None
        np.testing.assert_array_equal(out, _expect(mids, off, "mean", world))
        with dr.read_only_lookups():                 # the context does not yield to need_grad
            with pytest.raises(ValueError):
                eng.forward(torch.from_numpy(ids), need_grad=True)
        # the shards are what they were
        for tb, b0 in zip(be.tables, before):
            assert tb.keys() == b0.keys()
        open(os.path.join(outdir, "ok%d" % rank), "w").write("ok")
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_read_only_exchange_gloo():
    world = 2
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, _free_port(), d), nprocs=world, join=True)
        for r in range(world):
            assert os.path.exists(os.path.join(d, "ok%d" % r))
