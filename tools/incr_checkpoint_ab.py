"""Measurements of the incremental-checkpoint path, each in one process with
its two sides alternated three times (medians and run-to-run spreads):

  export  one table (2 M x 128 fp32 by default, filled by insert_synthetic)
          with 65 536 marked keys: export_updated() against the full export(),
          host clock around calls that end in a device synchronise.  The delta
          is checked against the filtered full export first.  With
          --kernel-stats (a rocprofv3 --kernel-trace --stats CSV of a run of
          this part) the scan kernel's achieved bytes / s over
          16 B x (cap + 1) is added.
  train   the bench's embedding train step (embedding_lookup_sparse_multi
          one-hot forward, backward, apply_gradients; eager) over T tables:
          tracking off against on by key (track_updates()) and on by row
          (track_updates(by_row=True)), for SGD and for Adagrad.  For SGD a
          fourth arm runs with tracking off and the fused backward + update
          disabled (the ordinary path a group tracked by key takes), so the
          loss of the fused path and the mark itself show separately; the
          marks of one step (grouped launches: by key, and by row over the
          forward's record-major rows) are also timed alone with device
          events.  With --kernel-stats (a rocprofv3 --kernel-trace --stats CSV
          of a run of this part) the device time of the two mark kernels is
          added.

  mark-stats  only reads --kernel-stats and prints the mark kernels' device
          time (the traced run is a run of its own, with few steps).

usage: python tools/incr_checkpoint_ab.py [--part export|train|all|mark-stats] [--rows 2000000]
           [--dim 128] [--marked 65536] [--train-tables 26] [--train-rows 4000000]
           [--batch 65536] [--steps 20] [--kernel-stats CSV] [--out profiles/incr_checkpoint.json]"""
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

ROUNDS = 3


def _summary(runs, nd=4):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def part_export(args, dr, dev):
    R, D, M = args.rows, args.dim, args.marked
    ev = dr.EmbeddingVariable("incr_ab", D, 0.0, device=dev, capacity=R)
    ev.insert_synthetic(0, R, seed=77)
    cap = dr._lib.lib().dr_ev_row_capacity(ev.handle)
    slots = 1
    while slots < 2 * max(1024, R):     # dr_ev_create's sizing of the slot table
        slots <<= 1
    ev.track_updates()
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    marked = torch.randperm(R, generator=g, device=dev)[:M]
    ev.mark_updated(marked)
    full = ev.export()
    delta = ev.export_updated()
    sel = torch.isin(full[0], marked)
    assert delta[0].numel() == M and torch.equal(delta[0], full[0][sel])
    assert torch.equal(delta[1].view(torch.int32), full[1][sel].view(torch.int32))
    del full, delta, sel
    t_delta, t_full = [], []
    for _ in range(ROUNDS):
        t_delta.append(_clock(ev.export_updated))
        t_full.append(_clock(ev.export))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_mark = []
    for _ in range(ROUNDS):
        ev.clear_updated()
        a.record()
        ev.mark_updated(marked)
        b.record()
        torch.cuda.synchronize()
        t_mark.append(a.elapsed_time(b))
    res = {"shape": {"rows": R, "dim": D, "marked": M, "row_capacity": cap, "slots": slots + 1},
           "export_updated_ms": _summary(t_delta), "export_full_ms": _summary(t_full),
           "mark_call_ms": _summary(t_mark, 5),
           "moved_bytes": {"delta_rows": M * D * 4, "full_rows": R * D * 4,
                           "scan": 16 * (slots + 1)}}
    res["full_over_delta"] = round(res["export_full_ms"]["median"]
                                   / res["export_updated_ms"]["median"], 2)
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "ev_scan_updated_kernel" in row.get("Name", ""):
                    ns = float(row["AverageNs"])
                    res["scan_kernel"] = {"avg_us": round(ns / 1e3, 2), "calls": int(row["Calls"]),
                                          "bytes": 16 * (slots + 1),
                                          "gb_per_s": round(16 * (slots + 1) / ns, 1)}
    return res


def part_train(args, dr, dev):
    import bench
    from deeprec_amd import embedding_ops as eo
    T, R, D, B = args.train_tables, args.train_rows, args.dim, args.batch
    evs = []
    for t in range(T):
        ev = dr.EmbeddingVariable("incr_tr%d" % t, D, 0.0, device=dev, capacity=R + (1 << 20))
        ev.insert_synthetic(0, R, seed=1000 + t)
        evs.append(ev)
    batches = bench.make_batches(4, T, B, R, 0.0, 91, dev)
    ind = torch.stack([torch.arange(B, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)],
                      1)
    sps = [[dr.SparseTensor(ind, ids[t], (B, 1)) for t in range(T)] for ids in batches]
    upstream = torch.randn((B, T * D), device=dev)

    def steps(opt, n):
        for i in range(n):
            out = dr.embedding_lookup_sparse_multi(evs, sps[i % len(sps)], combiner="sum")
            out.backward(upstream)
            opt.apply_gradients(evs)

    def track(on, by_row=False):
        for ev in evs:
            ev.track_updates(on, by_row=by_row)

    res = {"shape": {"tables": T, "rows": R, "dim": D, "batch": B, "steps": args.steps,
                     "graph": False}}
    for name, opt in (("sgd", dr.GradientDescentOptimizer(0.01)),
                      ("adagrad", dr.AdagradOptimizer(0.01))):
        arms = [("off", False, False, True), ("on", True, False, True),
                ("on_row", True, True, True)]
        if name == "sgd":
            arms.append(("off_unfused", False, False, False))
        steps(opt, 4)                      # every batch once: slots exist, code loaded
        per = {a[0]: [] for a in arms}
        for _ in range(ROUNDS):
            for arm, on, by_row, fused in arms:
                track(on, by_row)
                old, eo._FUSED_SGD = eo._FUSED_SGD, fused and eo._FUSED_SGD
                try:
                    steps(opt, 2)
                    per[arm].append(_clock(lambda: steps(opt, args.steps)) / args.steps)
                finally:
                    eo._FUSED_SGD = old
        track(False)
        res[name] = {arm + "_ms_per_step": _summary(v) for arm, v in per.items()}
        for arm in ("on", "on_row"):
            res[name][arm + "_minus_off_ms"] = round(res[name][arm + "_ms_per_step"]["median"]
                                                     - res[name]["off_ms_per_step"]["median"], 4)
        # an improvement: by key's on - off exceeds by row's by more than the two spreads added
        res[name]["row_saves_ms"] = round(res[name]["on_ms_per_step"]["median"]
                                          - res[name]["on_row_ms_per_step"]["median"], 4)
        res[name]["row_is_improvement"] = bool(
            res[name]["row_saves_ms"] > res[name]["on_ms_per_step"]["spread"]
            + res[name]["on_row_ms_per_step"]["spread"])
        if name == "sgd":
            res[name]["unfused_minus_fused_ms"] = round(
                res[name]["off_unfused_ms_per_step"]["median"]
                - res[name]["off_ms_per_step"]["median"], 4)
            res[name]["on_minus_unfused_ms"] = round(
                res[name]["on_ms_per_step"]["median"]
                - res[name]["off_unfused_ms_per_step"]["median"], 4)
    # one step's marks alone, as apply_gradients issues them (grouped: one
    # launch per 32 tables), device events
    from deeprec_amd.kv_variable_ops import mark_updated_grouped
    track(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_mark = []
    for r in range(ROUNDS + 1):
        ids = batches[r % len(batches)]
        a.record()
        mark_updated_grouped(evs, [ids[t] for t in range(T)])
        b.record()
        torch.cuda.synchronize()
        if r:
            t_mark.append(a.elapsed_time(b))
    res["mark_calls_per_step_ms"] = _summary(t_mark, 5)
    # ... and by row, as apply_gradients issues it for a fused group: one launch
    # over the forward's record-major rows, the gradient left unformed
    track(True, by_row=True)
    t_rows = []
    for r in range(ROUNDS + 1):
        out = dr.embedding_lookup_sparse_multi(evs, sps[r % len(sps)], combiner="sum")
        out.backward(upstream)
        pend = evs[0].pending_grads[-1]._pending
        assert pend.group.rows_record and pend.fusable()
        a.record()
        pend.mark_rows(evs, dr._lib.stream_handle(dev))
        b.record()
        torch.cuda.synchronize()
        assert pend.fusable()
        if r:
            t_rows.append(a.elapsed_time(b))
        for ev in evs:
            ev.pending_grads = []
    track(False)
    res["row_mark_call_per_step_ms"] = _summary(t_rows, 5)
    res["row_mark_bytes"] = 8 * T * B
    if args.kernel_stats:
        res.update(mark_kernel_stats(args.kernel_stats))
    return res


def mark_kernel_stats(path):
    """Device time of the two mark kernels from a rocprofv3 --kernel-trace
    --stats CSV of a run of the train part."""
    res = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for kern in ("ev_mark_updated_rows_kernel", "ev_mark_updated_kernel"):
                if kern + "(" in name or name.endswith(kern):
                    us = lambda k: round(float(row[k]) / 1e3, 2) if row.get(k) else None
                    res[kern] = {"avg_us": us("AverageNs"), "calls": int(row["Calls"]),
                                 "min_us": us("MinNs"), "max_us": us("MaxNs")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["export", "train", "all", "mark-stats"])
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--marked", type=int, default=65536)
    ap.add_argument("--train-tables", type=int, default=26)
    ap.add_argument("--train-rows", type=int, default=4_000_000,
                    help="rows per table (the Adagrad arm holds a second column of them)")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part == "mark-stats":      # the CSV alone: no device needed
        print(json.dumps({"train": mark_kernel_stats(args.kernel_stats)}), flush=True)
        return
    import deeprec_amd as dr
    dr.load()
    if not torch.cuda.is_available():
        raise SystemExit("incr_checkpoint_ab.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    res = {}
    if args.part in ("export", "all"):
        res["export"] = part_export(args, dr, dev)
    if args.part in ("train", "all"):
        res["train"] = part_train(args, dr, dev)
    dr.status_check(dev)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
