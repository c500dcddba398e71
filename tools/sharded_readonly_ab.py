"""A/B of the native sharded engines' training forward against their
read-only forward (DR_SHARDED_READ_ONLY), one process, world 1, one MI355X.

  python tools/sharded_readonly_ab.py [--out profiles/sharded_readonly_ab.json]
                                      [--kinds rccl,fixed,xgmi]

The shape is bench.py's native_engine leg (T = 26 tables, D = 128, B = 65536
one-hot ids per table, 12.5 M resident rows per table, uniform ids, eager
forwards, the XGMI kind's result left in the engine buffer).  Every id is
resident, so the training forward (need_grad=False: the code as it was before
the read-only forward existed) inserts nothing and both forwards return the
same rows; that is checked bit for bit before timing.  For each kind the two
forwards are timed in three alternating runs (training, read-only, training,
...), each run `--steps` forwards between two device synchronisations after
two warm-up forwards.  Reported per kind: the runs, their medians, the
training forward's min-max spread, and whether the read-only median is no
slower than the training median by more than that spread.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=26)
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kinds", default="rccl,fixed,xgmi")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_readonly_ab.json"))
    args = ap.parse_args()
    import torch

    import deeprec_amd as dr
    from deeprec_amd.sharded import Comm, NativeShardedLookup
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dr.load()
    T, D, B, R = args.tables, args.dim, args.batch, args.rows
    evs = []
    for t in range(T):
        ev = dr.EmbeddingVariable("ab%d" % t, D, 0.0, device=dev, capacity=R + (1 << 20))
        ev.insert_synthetic(0, R, seed=1000 + t)
        evs.append(ev)
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    batches = [torch.randint(0, R, (T, B), generator=g, device=dev, dtype=torch.int64)
               for _ in range(4)]
    torch.cuda.synchronize()
    counts = [int(ev.total_count()[0]) for ev in evs]
    comm = Comm.rccl(0, 1)
    res = {"what": "NativeShardedLookup forward, training (need_grad=False) vs read-only, "
                   "world 1, one process, eager; ms per forward",
           "shape": {"tables": T, "dim": D, "batch": B, "rows_per_table": R},
           "method": "%d alternating runs per kind (training, read-only, ...), %d forwards per "
                     "run between device synchronisations, 2 warm-up forwards; medians; spread = "
                     "max - min of the training runs" % (args.runs, args.steps),
           "device": torch.cuda.get_device_name(dev), "kinds": {}}

    def timed(eng, copy, ro):
        with torch.no_grad():
            for k in range(2):
                eng.forward(batches[k], combiner="sum", copy=copy, read_only=ro)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                eng.forward(batches[i % len(batches)], combiner="sum", copy=copy, read_only=ro)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3

    for kind in args.kinds.split(","):
        eng = NativeShardedLookup(comm, evs, dev, kind=kind, batch=B, max_ids=B)
        copy = kind != "xgmi"
        same = True
        with torch.no_grad():
            for b in batches:
                a = eng.forward(b, combiner="sum", copy=copy, read_only=False).clone()
                c = eng.forward(b, combiner="sum", copy=copy, read_only=True)
                same = same and torch.equal(a, c)
        train, ro = [], []
        for _ in range(args.runs):
            train.append(round(timed(eng, copy, False), 4))
            ro.append(round(timed(eng, copy, True), 4))
        torch.cuda.synchronize()
        eng.close()
        tm, rm = sorted(train)[len(train) // 2], sorted(ro)[len(ro) // 2]
        spread = round(max(train) - min(train), 4)
        res["kinds"][kind] = {
            "outputs_bit_equal": bool(same), "training_runs": train, "readonly_runs": ro,
            "training_median": tm, "readonly_median": rm, "training_spread": spread,
            "readonly_minus_training": round(rm - tm, 4),
            "readonly_no_slower_beyond_spread": bool(rm - tm <= spread)}
        print(kind, json.dumps(res["kinds"][kind]), flush=True)
    comm.close()
    dr.status_check()
    res["tables_unchanged"] = counts == [int(ev.total_count()[0]) for ev in evs]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
