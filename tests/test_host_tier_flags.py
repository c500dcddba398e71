"""The host store's colmask as a flag word: the five
entries an incremental checkpoint of a tiered key space needs --
dr_host_tier_count_masked / export_masked / clear_bits / or_bits / shrink_keys
-- against a Python dict, over seeded random walks mixed with put / take /
remove, the full export compared with the dict after every operation.  The
store and the key pool are tests/test_host_tier_store.py's (capacity_hint 1,
the special keys, a cluster on one home bucket, columns of 4, 32 and 10
bytes); colmask draws bits 0-2 and bit 16.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

from test_host_tier_store import (COL_BYTES, I64MAX, I64MIN, Store, check_export, entry,  # noqa: F401
                                  key_pool, lib)

UPDATED = 1 << 16
INVALID_ARGUMENT = 3


class FlagStore(Store):
    def count_masked(self, mask):
        n = C.c_int64(-1)
        assert self.lib.dr_host_tier_count_masked(self.t, mask, C.byref(n)) == 0
        return n.value

    def export_masked(self, mask):
        m = C.c_int64(-1)
        assert self.lib.dr_host_tier_export_masked(self.t, mask, None, None, None, None, None, 0,
                                                   C.byref(m)) == 0      # the count query
        n = m.value
        vals, ptrs = self._cols(n)
        keys, ver, frq = (np.zeros(n + 1, np.int64) for _ in range(3))
        cm = np.zeros(n + 1, np.uint32)
        assert self.lib.dr_host_tier_export_masked(self.t, mask, keys.ctypes.data, ptrs,
                                                   ver.ctypes.data, frq.ctypes.data,
                                                   cm.ctypes.data, n, C.byref(m)) == 0
        assert m.value == n
        for v, b in zip(vals, COL_BYTES):                   # nothing past the count is written
            assert (v[n] == 0xA5).all()
        return keys[:n], [v[:n] for v in vals], ver[:n], frq[:n], cm[:n]

    def clear_bits(self, mask):
        n = C.c_int64(-1)
        assert self.lib.dr_host_tier_clear_bits(self.t, mask, C.byref(n)) == 0
        return n.value

    def or_bits(self, keys, require, bits):
        n = C.c_int64(-1)
        assert self.lib.dr_host_tier_or_bits(self.t, keys.ctypes.data, keys.size, require, bits,
                                             C.byref(n)) == 0
        return n.value

    def shrink_keys(self, gs, stl, capacity=None):
        cap = self.size() if capacity is None else capacity
        out = np.full(cap + 1, -77, np.int64)
        n = C.c_int64(-1)
        rc = self.lib.dr_host_tier_shrink_keys(self.t, gs, stl, out.ctypes.data, cap, C.byref(n))
        return rc, out, n.value


def check_masked(store, model, mask):
    want = sorted(k for k, e in model.items() if (e[2] & mask) == mask)
    assert store.count_masked(mask) == len(want)
    keys, vals, ver, frq, cm = store.export_masked(mask)
    assert keys.tolist() == want                            # ascending as signed int64
    for j, k in enumerate(want):
        assert entry(vals, ver, frq, cm, j) == model[k], k
    return len(want)


@pytest.mark.parametrize("seed", [5, 67])
def test_flag_walk_matches_dict(lib, seed):
    rng = np.random.default_rng(seed)
    pool = key_pool(rng)
    store, model = FlagStore(lib), {}
    gs, peak = 0, 0
    seen = dict(masked=0, cleared=0, ored=0, shrunk=0, or_skipped=0)
    for op in range(600):
        kind = int(rng.integers(0, 14))
        n = int(rng.integers(0, 60))
        keys = np.ascontiguousarray(rng.choice(pool, n))    # with replacement: duplicates
        if op % 50 == 0:
            keys = np.array([-1, 0, I64MIN, I64MAX, -1], np.int64)
            n = keys.size
        if kind < 5:
            vals = [rng.integers(0, 256, (n, b)).astype(np.uint8) for b in COL_BYTES]
            ver = np.where(rng.random(n) < 0.2, -1, rng.integers(0, 64, n)).astype(np.int64)
            frq = rng.integers(0, 9, n).astype(np.int64)
            cm = (rng.integers(0, 8, n) | (rng.integers(0, 2, n) << 16)).astype(np.uint32)
            store.put(keys, vals, ver, frq, cm)
            for j, k in enumerate(keys.tolist()):
                model[k] = entry(vals, ver, frq, cm, j)
        elif kind < 6:
            idx, vals, ver, frq, cm = store.take(keys, 1)
            hit = {k for k in keys.tolist() if k in model}
            assert idx.size == len(hit)
            for j, i in enumerate(idx.tolist()):            # bit 16 comes back with the entry
                assert entry(vals, ver, frq, cm, j) == model[int(keys[i])]
            for k in hit:
                del model[k]
        elif kind < 7:
            gone = {k for k in keys.tolist() if k in model}
            assert store.remove(keys) == len(gone)
            for k in gone:
                del model[k]
        elif kind < 9:                                      # or_bits: require the primary bit
            require, bits = (1, UPDATED) if rng.random() < 0.7 else (int(rng.integers(0, 8)), 4)
            hit = {k for k in keys.tolist() if k in model and (model[k][2] & require) == require}
            seen["or_skipped"] += sum(k in model for k in set(keys.tolist())) - len(hit)
            assert store.or_bits(keys, require, bits) == len(hit)
            for k in hit:
                e = model[k]
                model[k] = e[:2] + (e[2] | bits,) + e[3:]
            seen["ored"] += len(hit)
        elif kind < 10:                                     # clear_bits
            mask = UPDATED if rng.random() < 0.7 else int(rng.integers(1, 8))
            changed = [k for k, e in model.items() if e[2] & mask]
            assert store.clear_bits(mask) == len(changed)
            for k in changed:
                e = model[k]
                model[k] = e[:2] + (e[2] & ~mask,) + e[3:]
            seen["cleared"] += len(changed)
        elif kind < 12:                                     # shrink_keys
            gs += int(rng.integers(0, 8))
            stl = int(rng.integers(8, 48))
            dropped = set()
            for k in list(model):
                e = model[k]
                if e[0] == -1:
                    model[k] = (gs,) + e[1:]
                elif gs - e[0] > stl:
                    del model[k]
                    dropped.add(k)
            rc, out, r = store.shrink_keys(gs, stl)
            assert rc == 0 and r == len(dropped)
            assert set(out[:r].tolist()) == dropped and len(set(out[:r].tolist())) == r
            assert (out[r:] == -77).all()
            seen["shrunk"] += r
        else:                                               # the masked reads, several masks
            for mask in (UPDATED, UPDATED | 1, UPDATED | 1 | 2, UPDATED | 1 | 4, 0, 3):
                seen["masked"] += check_masked(store, model, mask)
        check_export(store, model)
        peak = max(peak, len(model))
    check_masked(store, model, UPDATED | 1)
    store.close()
    # the walk went where it was meant to
    assert peak > 8 * 0.75 * 2 ** 4, peak
    assert min(seen.values()) > 20, seen


def test_flag_refusals(lib):
    store = FlagStore(lib)
    rng = np.random.default_rng(9)
    n = 40
    keys = np.arange(n, dtype=np.int64) * 7 - 100
    vals = [rng.integers(0, 256, (n, b)).astype(np.uint8) for b in COL_BYTES]
    ver = np.where(np.arange(n) % 5 == 0, -1, 3).astype(np.int64)     # 8 unstamped, 32 old
    frq = np.ones(n, np.int64)
    cm = np.full(n, UPDATED | 1, np.uint32)
    store.put(keys, vals, ver, frq, cm)
    model = {int(k): entry(vals, ver, frq, cm, j) for j, k in enumerate(keys)}

    # export_masked: a small capacity writes nothing and reports the count
    m = C.c_int64(-1)
    out = np.full(n, -77, np.int64)
    assert lib.dr_host_tier_export_masked(store.t, UPDATED, out.ctypes.data, None, None, None,
                                          None, n - 1, C.byref(m)) == INVALID_ARGUMENT
    assert m.value == n and (out == -77).all()
    # shrink_keys: a capacity under size() is refused before a version is stamped or a key goes
    rc, out, _ = store.shrink_keys(100, 10, capacity=n - 1)
    assert rc == INVALID_ARGUMENT and (out == -77).all()
    check_export(store, model)
    rc, out, r = store.shrink_keys(100, 10)                 # and with room it runs: 32 go
    assert rc == 0 and r == 32 and store.size() == 8
    # null handle, null count
    z = C.c_int64(0)
    assert lib.dr_host_tier_count_masked(None, 1, C.byref(z)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_count_masked(store.t, 1, None) == INVALID_ARGUMENT
    assert lib.dr_host_tier_export_masked(None, 1, None, None, None, None, None, 0,
                                          C.byref(z)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_clear_bits(None, 1, C.byref(z)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_or_bits(None, keys.ctypes.data, 1, 1, 1, C.byref(z)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_or_bits(store.t, None, 1, 1, 1, C.byref(z)) == INVALID_ARGUMENT
    assert lib.dr_host_tier_shrink_keys(None, 0, 1, out.ctypes.data, 99, C.byref(z)) == \
        INVALID_ARGUMENT
    # nullable counts
    assert lib.dr_host_tier_clear_bits(store.t, UPDATED, None) == 0
    assert store.count_masked(UPDATED) == 0
    assert lib.dr_host_tier_or_bits(store.t, keys.ctypes.data, n, 1, UPDATED, None) == 0
    assert store.count_masked(UPDATED) == 8
    store.close()
