"""The host-DRAM tier's store (deeprec-1_amd/csrc/dr_host_tier.h through the
dr_host_tier_* entries) against a Python dict: seeded random walks of put /
take (erase 0 and 1) / remove / shrink, the full export compared with the dict
after every operation.  The store starts at capacity_hint=1, so its map
rehashes several times; the key pool holds -1, 0, INT64_MIN, INT64_MAX and a
few hundred keys that share one home bucket; a take names keys twice; the
three columns are 4, 32 and 10 bytes wide.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deeprec-1_amd", "deeprec_amd", "libdeeprec_amd.so")
COL_BYTES = (4, 32, 10)
I64MIN, I64MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "deeprec-1_amd")])
    import deeprec_amd._lib as L
    lib = C.CDLL(LIB)
    for name, (res, args) in L.SIGNATURES.items():
        if name.startswith("dr_host_tier_"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def mix64(k):
    k = np.asarray(k).astype(np.uint64)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    return k ^ (k >> np.uint64(33))


def key_pool(rng):
    special = np.array([-1, 0, I64MIN, I64MAX, 1, -2], np.int64)
    cand = rng.integers(I64MIN, I64MAX, 1 << 20, dtype=np.int64, endpoint=True)
    with np.errstate(over="ignore"):
        same = cand[(mix64(cand) & np.uint64(4095)) == np.uint64(77)][:300]   # one home bucket
    assert same.size >= 200
    pool = np.unique(np.concatenate([special, same, cand[:600]]))
    assert np.isin(special, pool).all()
    return pool


class Store(object):
    def __init__(self, lib):
        self.lib = lib
        self.t = C.c_void_p()
        cb = (C.c_int64 * 3)(*COL_BYTES)
        assert lib.dr_host_tier_create(3, cb, 1, C.byref(self.t)) == 0

    def close(self):
        assert self.lib.dr_host_tier_destroy(self.t) == 0

    @staticmethod
    def _cols(n):
        vals = [np.full((n + 1, b), 0xA5, np.uint8) for b in COL_BYTES]
        return vals, (C.c_void_p * 3)(*[v.ctypes.data for v in vals])

    def size(self):
        n = C.c_int64(-1)
        assert self.lib.dr_host_tier_size(self.t, C.byref(n)) == 0
        return n.value

    def put(self, keys, vals, ver, frq, cm):
        ptrs = (C.c_void_p * 3)(*[v.ctypes.data for v in vals])
        assert self.lib.dr_host_tier_put(self.t, keys.ctypes.data, keys.size, ptrs,
                                         ver.ctypes.data, frq.ctypes.data, cm.ctypes.data) == 0

    def take(self, keys, erase):
        n = keys.size
        vals, ptrs = self._cols(n)
        idx, ver, frq = (np.full(n + 1, -7, np.int64) for _ in range(3))
        cm = np.zeros(n + 1, np.uint32)
        hits = C.c_int64(-1)
        assert self.lib.dr_host_tier_take(self.t, keys.ctypes.data, n, erase, idx.ctypes.data, ptrs,
                                          ver.ctypes.data, frq.ctypes.data, cm.ctypes.data,
                                          C.byref(hits)) == 0
        h = hits.value
        return idx[:h], [v[:h] for v in vals], ver[:h], frq[:h], cm[:h]

    def remove(self, keys):
        n = C.c_int64(-1)
        assert self.lib.dr_host_tier_remove(self.t, keys.ctypes.data, keys.size, C.byref(n)) == 0
        return n.value

    def shrink(self, gs, stl):
        n = C.c_int64(-1)
        assert self.lib.dr_host_tier_shrink(self.t, gs, stl, C.byref(n)) == 0
        return n.value

    def export(self):
        m = C.c_int64(-1)
        assert self.lib.dr_host_tier_export(self.t, None, None, None, None, None, 0,
                                            C.byref(m)) == 0
        n = m.value
        vals, ptrs = self._cols(n)
        keys, ver, frq = (np.zeros(n + 1, np.int64) for _ in range(3))
        cm = np.zeros(n + 1, np.uint32)
        assert self.lib.dr_host_tier_export(self.t, keys.ctypes.data, ptrs, ver.ctypes.data,
                                            frq.ctypes.data, cm.ctypes.data, n, C.byref(m)) == 0
        assert m.value == n
        return keys[:n], [v[:n] for v in vals], ver[:n], frq[:n], cm[:n]


def entry(vals, ver, frq, cm, j):
    return (int(ver[j]), int(frq[j]), int(cm[j])) + tuple(v[j].tobytes() for v in vals)


def check_export(store, model):
    keys, vals, ver, frq, cm = store.export()
    want = sorted(model)                                    # Python ints: signed order
    assert store.size() == len(want)
    assert keys.tolist() == want
    for j, k in enumerate(want):
        assert entry(vals, ver, frq, cm, j) == model[k], k


@pytest.mark.parametrize("seed", [3, 41])
def test_store_walk_matches_dict(lib, seed):
    rng = np.random.default_rng(seed)
    pool = key_pool(rng)
    store, model = Store(lib), {}
    gs, peak, dup_takes = 0, 0, 0
    for op in range(700):
        kind = int(rng.integers(0, 10))
        n = int(rng.integers(0, 60))
        keys = np.ascontiguousarray(rng.choice(pool, n))    # with replacement: duplicates
        if op % 50 == 0:
            keys = np.array([-1, 0, I64MIN, I64MAX, -1], np.int64)
            n = keys.size
        if kind < 5:
            vals = [rng.integers(0, 256, (n, b)).astype(np.uint8) for b in COL_BYTES]
            ver = np.where(rng.random(n) < 0.2, -1, rng.integers(0, 64, n)).astype(np.int64)
            frq = rng.integers(0, 9, n).astype(np.int64)
            cm = rng.integers(0, 8, n).astype(np.uint32)
            store.put(keys, vals, ver, frq, cm)
            for j, k in enumerate(keys.tolist()):           # the last occurrence wins
                model[k] = entry(vals, ver, frq, cm, j)
        elif kind < 7:
            erase = int(rng.integers(0, 2))
            idx, vals, ver, frq, cm = store.take(keys, erase)
            first = {}
            for i, k in enumerate(keys.tolist()):
                if k in model and k not in first:
                    first[k] = i
            dup_takes += len(first) < sum(k in model for k in keys.tolist())
            assert idx.tolist() == sorted(first.values())   # compacted, in input order
            for j, i in enumerate(idx.tolist()):
                assert entry(vals, ver, frq, cm, j) == model[int(keys[i])]
            if erase:
                for k in first:
                    del model[k]
        elif kind < 9:
            gone = {k for k in keys.tolist() if k in model}
            assert store.remove(keys) == len(gone)
            for k in gone:
                del model[k]
        else:
            gs += int(rng.integers(0, 8))
            stl = int(rng.integers(8, 48))
            dropped = 0
            for k in list(model):
                e = model[k]
                if e[0] == -1:
                    model[k] = (gs,) + e[1:]                # stamped and kept
                elif gs - e[0] > stl:
                    del model[k]
                    dropped += 1
            assert store.shrink(gs, stl) == dropped
        check_export(store, model)
        peak = max(peak, len(model))
    store.close()
    # the walk went where it was meant to: several rehashes from 8 buckets
    # (the map doubles at 3/4), the special keys stored, repeated keys taken
    assert peak > 8 * 0.75 * 2 ** 4, peak
    assert dup_takes > 10
