"""Measurement of keyed removal and the removal log: remove() of 65 536 keys
and of every second key, next to the shrink() that evicts the same second
half on a twin table (the same mark + rehash, the yardstick), and shrink()
with the removal log on against off.  One table shape (4 M x 128 fp32 with an
Adagrad slot column by default), fresh tables for every case and round
(medians and run-to-run spreads), host clock around calls that end in a device
synchronise.  Every result is checked first: the count returned, the key
count, and find() on sampled keys.

With --kernel-stats (the rocprofv3 --kernel-trace --stats CSV of a run of
this tool with --rounds 1 --cases big,shrink_log, so that each of the two new
kernels runs once) ev_remove_mark_kernel and ev_collect_dropped_kernel are set
against the bytes they must move and the 8 TB/s HBM peak:
  mark    : per key the 8-B key, one 16-B slot and the 4-B word of `keep`
  collect : 1 B x (cap + 1) of `keep`, and per dropped key its 8-B key read
            and its 8-B log entry written

usage: python tools/remove_ab.py [--rows 4000000] [--dim 128] [--rounds 3]
           [--cases small,big,shrink,shrink_log] [--kernel-stats CSV]
           [--out profiles/remove.json]"""
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
SMALL = 65536
HBM_PEAK_GBS = 8000.0
CASES = ("small", "big", "shrink", "shrink_log")


def _summary(runs, nd=3):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _table(args, dr, dev, name, versions):
    R, D = args.rows, args.dim
    ev = dr.EmbeddingVariable(name, D, 0.0, steps_to_live=1, device=dev, capacity=R)
    acc = ev.slot("Adagrad", 0.1)
    ev.insert_synthetic(0, R, seed=77)
    acc.insert_synthetic(0, R, seed=78)
    if versions:
        # odd keys get the current step and stay; even keys keep version 0 and go
        odd = torch.arange(1, R, 2, dtype=torch.int64, device=dev)
        step = 1 << 18
        zeros = torch.zeros((step, D), device=dev)
        for i in range(0, odd.numel(), step):    # existing rows are kept: only the version lands
            part = odd[i:i + step]
            ev.insert(part, zeros[:part.numel()], torch.full_like(part, GS))
    return ev


def _check(ev, R, gone_mask_of, removed, expect, sample):
    assert removed == expect, (removed, expect)
    assert int(ev.total_count()[0]) == R - expect and ev.rows_allocated() == R
    rows = ev.find(sample)
    assert torch.equal(rows < 0, gone_mask_of(sample))


def one_case(args, dr, dev, case, r):
    R = args.rows
    g = torch.Generator(device=dev)
    g.manual_seed(3 + r)
    sample = torch.randint(0, R, (1 << 16,), generator=g, device=dev)
    ev = _table(args, dr, dev, "remove_ab_%s_%d" % (case, r), case.startswith("shrink"))
    even = lambda k: k % 2 == 0
    if case == "small":
        keys = torch.randperm(R, generator=g, device=dev)[:SMALL].to(torch.int64)
        t, n = _clock(lambda: ev.remove(keys))
        gone = torch.zeros(R, dtype=torch.bool, device=dev)
        gone[keys] = True
        _check(ev, R, lambda k: gone[k], n, SMALL, sample)
    elif case == "big":
        keys = torch.arange(0, R, 2, dtype=torch.int64, device=dev)
        keys = keys[torch.randperm(keys.numel(), generator=g, device=dev)]   # a caller's order
        t, n = _clock(lambda: ev.remove(keys))
        _check(ev, R, even, n, (R + 1) // 2, sample)
    else:
        if case == "shrink_log":
            ev.track_removals()
        t, n = _clock(lambda: ev.shrink(GS))
        _check(ev, R, even, n, (R + 1) // 2, sample)
        if case == "shrink_log":
            assert ev.removed_count() == n
            got = ev.export_removed()
            assert torch.equal(got, torch.arange(0, R, 2, dtype=torch.int64, device=dev))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [c for c in args.cases.split(",") if c]
    assert all(c in CASES for c in cases), cases
    if args.kernel_stats and not os.path.exists(args.kernel_stats):
        raise SystemExit("no such file: %s" % args.kernel_stats)
    import deeprec_amd as dr
    dr.load()
    if not torch.cuda.is_available():
        raise SystemExit("remove_ab.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    R, D = args.rows, args.dim
    slots = 1
    while slots < 2 * max(1024, R):     # dr_ev_create's sizing of the slot table
        slots <<= 1
    times = {c: [] for c in cases}
    for r in range(args.rounds):
        for c in cases:                 # the cases alternate inside a round
            times[c].append(one_case(args, dr, dev, c, r))
    big = (R + 1) // 2
    names = {"small": "remove_%d_ms" % SMALL, "big": "remove_%d_ms" % big,
             "shrink": "shrink_%d_ms" % big, "shrink_log": "shrink_%d_log_on_ms" % big}
    res = {"shape": {"rows": R, "dim": D, "columns": 2, "slots": slots + 1}}
    for c in cases:
        res[names[c]] = _summary(times[c])
    res["bytes"] = {"mark_per_key": 8 + 16 + 4, "mark_%d" % big: big * (8 + 16 + 4),
                    "collect_%d" % big: (slots + 1) + big * 16,
                    "rehash_scan": 17 * (slots + 1)}
    if args.kernel_stats:
        kern = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in ("ev_remove_mark_kernel", "ev_collect_dropped_kernel",
                          "ev_shrink_mark_kernel", "ev_rehash_kept_kernel"):
                    if k in name:
                        kern[k] = {"avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                   "calls": int(row["Calls"])}
        if "ev_remove_mark_kernel" in kern:
            kern["ev_remove_mark_kernel"]["bytes"] = big * (8 + 16 + 4)
        if "ev_collect_dropped_kernel" in kern:
            kern["ev_collect_dropped_kernel"]["bytes"] = (slots + 1) + big * 16
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
