"""Measurement of the EV key budget at save time: shrink_to() next to
remove() of the same victim list, precomputed on the host side, on a twin
table -- the floor (mark + rehash + removal log) -- so that the difference is
the cost of choosing the victims on the device (gather + radix select + mark).
One table (4 M x 128 fp32 by default, --rows 12500000 for the headline
table), versions drawn from 1 000 distinct steps, 10 % and 50 % eviction,
three fresh table pairs one after another (medians and run-to-run spreads),
host clock around calls that end in a device synchronise, removal log on.
The evicted table is checked first: its keys are exactly the twin's.

The selection's time is set against the bytes it must move: 16 B x (cap + 1)
slots for the gather, one 8-B metric read per live row (a gather by row:
counted both as 8 B and as a whole 128-B line), 20 B written per live key,
the candidate bytes of the 16 select passes (replayed here on the same
versions, skipped passes and compaction decisions included) and 20 B per live
key for the mark.

With --kernel-stats (the rocprofv3 --kernel-trace --stats CSV of a run of
this tool, --rounds 1) the average time and the calls of the kernels of both
paths are added: where the selection's time goes.

usage: python tools/budget_evict_ab.py [--rows 4000000] [--dim 128] [--rounds 3]
           [--kernel-stats CSV] [--out profiles/budget_evict.json]"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

STEPS = 1000
HBM_PEAK_GBS = 8000.0
LINE = 128
I64MIN = -(1 << 63)


def _summary(runs, nd=3):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _table(dr, dev, name, R, D, versions):
    ev = dr.EmbeddingVariable(name, D, 0.0, steps_to_live=10**9, device=dev, capacity=R)
    ev.insert_synthetic(0, R, seed=77)
    keys = torch.arange(0, R, dtype=torch.int64, device=dev)
    step = 1 << 18
    zeros = torch.zeros((step, D), device=dev)
    for i in range(0, R, step):                # existing rows are kept: only the version lands
        part = keys[i:i + step]
        ev.insert(part, zeros[:part.numel()], versions[i:i + step])
    ev.track_removals()
    return ev


def select_bytes(m, k, E):
    """Replays the select's 16 passes on the biased (metric, key) words:
    entries read per pass, bytes read and written."""
    read = written = 0
    per_pass = []
    match = torch.ones_like(m, dtype=torch.bool)
    compact, rank = False, E
    # the bits in which some live entries differ: the pass of a digit without one is skipped
    diff = []
    for w in (m, k):
        a = w.cpu().numpy()
        diff.append(int(np.bitwise_and.reduce(a) ^ np.bitwise_or.reduce(a)) & ((1 << 64) - 1))
    for d in range(16):
        n_buf = m.numel()
        if not compact and (diff[d >> 3] >> (56 - 8 * (d & 7))) & 255 == 0:
            per_pass.append(0)
            continue
        if compact:
            m, k = m[match], k[match]
            match = torch.ones_like(m, dtype=torch.bool)
            read += 16 * n_buf
            written += 16 * m.numel()
        else:
            read += (8 if d < 8 else 16) * n_buf
        per_pass.append(n_buf)
        shift = 56 - 8 * (d & 7)
        digit = ((m if d < 8 else k) >> shift) & 255
        hist = torch.bincount(digit[match], minlength=256).cpu()
        below, chosen = 0, 255
        for b in range(256):
            if below + int(hist[b]) >= rank:
                chosen = b
                break
            below += int(hist[b])
        rank -= below
        match = match & (digit == chosen)
        compact = d < 14 and 2 * int(hist[chosen]) <= m.numel()
    return {"entries_read_per_pass": per_pass, "read": read, "written": written}


def one_pair(args, dr, dev, r, frac):
    R, D = args.rows, args.dim
    g = torch.Generator(device=dev)
    g.manual_seed(11 + r)
    versions = torch.randint(1, STEPS + 1, (R,), generator=g, device=dev, dtype=torch.int64)
    E = int(R * frac)
    # keys are 0 .. R-1: (version, key) ascending is version * R + key ascending
    order = torch.sort(versions * R + torch.arange(R, device=dev, dtype=torch.int64))[0]
    victims = (order[:E] % R).contiguous()
    del order
    a = _table(dr, dev, "budget_ab_a_%d_%d" % (r, int(frac * 100)), R, D, versions)
    b = _table(dr, dev, "budget_ab_b_%d_%d" % (r, int(frac * 100)), R, D, versions)
    t_sel, n_a = _clock(lambda: a.shrink_to(R - E, "lru"))
    t_rm, n_b = _clock(lambda: b.remove(victims))
    assert n_a == E == n_b, (n_a, n_b, E)
    ka, kb = a.export()[0], b.export()[0]
    assert torch.equal(ka, kb) and ka.numel() == R - E
    assert torch.equal(a.export_removed(), b.export_removed())
    model = None
    if r == 0:
        keys = torch.arange(R, device=dev, dtype=torch.int64)
        model = select_bytes(versions ^ I64MIN, keys ^ I64MIN, E)
    del a, b
    dr.flush_releases()
    torch.cuda.empty_cache()
    return t_sel, t_rm, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import deeprec_amd as dr
    dr.load()
    if not torch.cuda.is_available():
        raise SystemExit("budget_evict_ab.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    R, D = args.rows, args.dim
    slots = 1
    while slots < 2 * max(1024, R):     # dr_ev_create's sizing of the slot table
        slots <<= 1
    res = {"shape": {"rows": R, "dim": D, "slots": slots + 1, "distinct_versions": STEPS}}
    # first use of both paths (code objects, the stream's memory pool) stays out of the clock
    warm = argparse.Namespace(rows=1 << 16, dim=D)
    one_pair(warm, dr, dev, 99, 0.5)
    for frac in (0.1, 0.5):
        ts, tr, model = [], [], None
        for r in range(args.rounds):
            a, b, m = one_pair(args, dr, dev, r, frac)
            ts.append(a)
            tr.append(b)
            model = model or m
        sel = [x - y for x, y in zip(ts, tr)]
        fixed = {"gather_slots": 16 * (slots + 1), "metric_8B": 8 * R, "metric_lines": LINE * R,
                 "gather_write": 20 * R, "mark": 20 * R}
        lo = (fixed["gather_slots"] + fixed["metric_8B"] + fixed["gather_write"] + fixed["mark"] +
              model["read"] + model["written"])
        hi = lo - fixed["metric_8B"] + fixed["metric_lines"]
        med = statistics.median(sel)
        res["evict_%d_pct" % int(frac * 100)] = {
            "evicted": int(R * frac),
            "shrink_to_ms": _summary(ts), "remove_ms": _summary(tr), "selection_ms": _summary(sel),
            "bytes": dict(fixed, select=model, total_low=lo, total_high=hi),
            "at_hbm_peak_ms": {"low": round(lo / HBM_PEAK_GBS / 1e6, 3),
                               "high": round(hi / HBM_PEAK_GBS / 1e6, 3)},
            "selection_gb_per_s": {"low": round(lo / (med * 1e6), 1),
                                   "high": round(hi / (med * 1e6), 1)} if med > 0 else None}
    if args.kernel_stats:
        kern = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in ("ev_budget_gather", "ev_select_init", "ev_select_pass", "ev_select_pick",
                          "ev_budget_mark", "ev_remove_mark", "ev_rehash_kept",
                          "ev_collect_dropped"):
                    if k + "_kernel" in name:
                        kern[k] = {"avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                   "calls": int(row["Calls"])}
        res["kernels"] = kern
    dr.status_check(dev)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
