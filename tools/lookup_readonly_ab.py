"""A/B of the fused one-hot lookups in one process, at the headline shape (26
EVs x 12.5 M x 128 fp32 filled by insert_synthetic, B = 65 536, four rotating
batches, all ids present): dr_ev_lookup_onehot_ex (training: zero-fill +
lookup kernel + miss kernel) and dr_ev_lookup_onehot_readonly (one kernel)
alternate call by call; each call is bracketed by device events.  Per round
the median call time of each; reported: the median over rounds and the
run-to-run spread (max - min of the per-round medians).  Then the read-only
call alone with 10 % absent ids.  The yardstick is the training call of the
same run.

usage: python tools/lookup_readonly_ab.py [--rows 12500000] [--tables 26] [--dim 128]
                                          [--batch 65536] [--iters 200] [--rounds 5]
                                          [--out profiles/readonly_ab.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--tables", type=int, default=26)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=200, help="calls of each kind per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    import deeprec_amd as dr
    from deeprec_amd._lib import check, lib, ptr, stream_handle, workspace
    dr.load()
    dev = torch.device("cuda:0")
    T, D, R, B = args.tables, args.dim, args.rows, args.batch
    evs = []
    for t in range(T):
        ev = dr.EmbeddingVariable("ab%d" % t, D, 0.0, device=dev, capacity=R + (1 << 20))
        ev.insert_synthetic(0, R, seed=1000 + t)
        evs.append(ev)
    handles = (C.c_void_p * T)(*[e.handle.value for e in evs])
    batches = bench.make_batches(4, T, B, R, 0.0, 91, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    absent = []
    for ids in batches:      # 10 % of the ids moved past the key space
        m = torch.rand(ids.shape, generator=g, device=dev) < 0.1
        absent.append(torch.where(m, ids + R + (1 << 21), ids))
    out = torch.empty((B, T * D), dtype=torch.float32, device=dev)
    wsb = lib().dr_ev_lookup_onehot_workspace_size(T, B)
    ws = workspace(wsb, dev)
    st = stream_handle(dev)
    L = lib()

    def train(ids):
        check(L.dr_ev_lookup_onehot_ex(handles, T, ptr(ids), 1, B, B, ptr(out), T * D, 0, 0, None,
                                       ptr(ws), wsb, st))

    def ro(ids):
        check(L.dr_ev_lookup_onehot_readonly(handles, T, ptr(ids), 1, B, B, ptr(out), T * D, 0, 0,
                                             None, st))

    def timed(fn, ids):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(ids)
        b.record()
        return a, b

    # both give the same bytes before anything is timed
    train(batches[0])
    ref = out.clone()
    ro(batches[0])
    assert torch.equal(ref.view(torch.int32), out.view(torch.int32))
    size0 = [int(e.total_count()[0]) for e in evs]
    for ids in batches:
        train(ids)
        ro(ids)
    torch.cuda.synchronize()

    def rounds(pairs):
        """pairs: [(name, fn, batch list)], alternated call by call."""
        per = {name: [] for name, _, _ in pairs}
        for _ in range(args.rounds):
            evts = {name: [] for name, _, _ in pairs}
            for i in range(args.iters):
                for name, fn, bl in pairs:
                    evts[name].append(timed(fn, bl[i % len(bl)]))
            torch.cuda.synchronize()
            for name in evts:
                per[name].append(statistics.median(a.elapsed_time(b) for a, b in evts[name]))
        return {name: {"median_ms": round(statistics.median(v), 5),
                       "spread_ms": round(max(v) - min(v), 5),
                       "round_medians_ms": [round(x, 5) for x in v]} for name, v in per.items()}

    res = {"shape": {"tables": T, "rows": R, "dim": D, "batch": B, "iters": args.iters,
                     "rounds": args.rounds},
           "all_present": rounds([("training", train, batches), ("readonly", ro, batches)]),
           "readonly_10pct_absent": rounds([("readonly", ro, absent)])["readonly"]}
    assert [int(e.total_count()[0]) for e in evs] == size0      # nothing was created
    ap_ = res["all_present"]
    res["readonly_minus_training_ms"] = round(ap_["readonly"]["median_ms"]
                                              - ap_["training"]["median_ms"], 5)
    per = 8 + 16 + 2 * 4 * D
    res["readonly_frac_of_peak_hbm"] = round(
        T * B * per / (ap_["readonly"]["median_ms"] * 1e-3) / 1e9 / bench.PEAK_HBM_GBS, 4)
    dr.status_check(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
