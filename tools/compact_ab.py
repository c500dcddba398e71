"""Measurement of EV row compaction at save time: compact() next to the
shrink() that precedes it and the export() that follows it, on one table
(4 M x 128 fp32 with an Adagrad slot column by default, every second key
evicted), three fresh tables one after another (medians and run-to-run
spreads), host clock around calls that end in a device synchronise.  The
compacted table is checked first: the live count, and a read-only gather of
sampled keys against the same gather before the compaction.

With --kernel-stats (the rocprofv3 --kernel-trace --stats CSV of a run of
this tool, --rounds 1) the live / slots / move kernels' times are set against
the bytes they must move -- 16 B x (cap + 1) slots per scan, 2 x rows moved x
row bytes x columns for the move -- and the 8 TB/s HBM peak.

usage: python tools/compact_ab.py [--rows 4000000] [--dim 128] [--rounds 3]
           [--kernel-stats CSV] [--out profiles/compact.json]"""
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

import torch  # noqa: E402

GS = 10
HBM_PEAK_GBS = 8000.0


def _summary(runs, nd=3):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def one_table(args, dr, dev, r):
    R, D = args.rows, args.dim
    ev = dr.EmbeddingVariable("compact_ab_%d" % r, D, 0.0, steps_to_live=1, device=dev, capacity=R)
    acc = ev.slot("Adagrad", 0.1)
    ev.insert_synthetic(0, R, seed=77)
    acc.insert_synthetic(0, R, seed=78)
    # odd keys get the current step and stay; even keys keep version 0 and go
    odd = torch.arange(1, R, 2, dtype=torch.int64, device=dev)
    step = 1 << 18
    zeros = torch.zeros((step, D), device=dev)
    for i in range(0, odd.numel(), step):      # existing rows are kept: only the version lands
        part = odd[i:i + step]
        ev.insert(part, zeros[:part.numel()], torch.full_like(part, GS))
    del zeros
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    sample = torch.randint(0, R, (1 << 16,), generator=g, device=dev)
    t_shrink, removed = _clock(lambda: ev.shrink(GS))
    assert removed == (R + 1) // 2, removed
    want = (ev.sparse_read(sample, read_only=True), acc.sparse_read(sample, read_only=True))
    rows = ev.find(sample)
    L = R - removed
    moved = int((ev.find(odd) >= L).sum())     # live rows at or above the live count
    t_compact, reclaimed = _clock(ev.compact)
    assert reclaimed == removed and ev.rows_allocated() == L == int(ev.total_count()[0])
    got = (ev.sparse_read(sample, read_only=True), acc.sparse_read(sample, read_only=True))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    new_rows = ev.find(sample)
    live = rows >= 0
    assert torch.equal(new_rows[~live], rows[~live]) and bool((new_rows[live] < L).all())
    stay = rows[live] < L
    assert torch.equal(new_rows[live][stay], rows[live][stay]) and moved > 0
    t_export, ex = _clock(ev.export)
    assert ex[0].numel() == L
    return t_shrink, t_compact, t_export, L, moved


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
        raise SystemExit("compact_ab.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    R, D = args.rows, args.dim
    slots = 1
    while slots < 2 * max(1024, R):     # dr_ev_create's sizing of the slot table
        slots <<= 1
    ts, tc, te, mv, L = [], [], [], [], 0
    for r in range(args.rounds):
        a, b, c, L, m = one_table(args, dr, dev, r)
        ts.append(a)
        tc.append(b)
        te.append(c)
        mv.append(m)
    moved = int(statistics.median(mv))   # (rows are numbered by racing inserts: it varies a little)
    res = {"shape": {"rows": R, "dim": D, "columns": 2, "evicted": R - L, "live": L,
                     "slots": slots + 1},
           "shrink_ms": _summary(ts), "compact_ms": _summary(tc), "export_ms": _summary(te),
           "rows_moved": mv,
           "bytes": {"slot_scan": 16 * (slots + 1), "row": D * 4, "move": 2 * moved * D * 4 * 2}}
    if args.kernel_stats:
        kern = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in ("live", "count", "rank", "move", "dirty", "slots", "tail"):
                    if "ev_compact_%s_kernel" % k in name:
                        kern[k] = {"avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                   "calls": int(row["Calls"])}
        for k in ("live", "slots"):
            if k in kern:
                kern[k]["bytes"] = 16 * (slots + 1)
        if "move" in kern:   # (this run's count; the profiled run builds its table the same way)
            kern["move"]["bytes"] = 2 * moved * D * 4 * 2
        for k in kern.values():
            if "bytes" in k:
                k["gb_per_s"] = round(k["bytes"] / (k["avg_us"] * 1e3), 1)
                k["of_hbm_peak"] = round(k["gb_per_s"] / HBM_PEAK_GBS, 3)
        res["kernels"] = kern
    dr.status_check(dev)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
