"""Measurement of dense update tracking and dense deltas on
section 21's shape: 8 dense tables of 3 536 rows, D = 128, 65 536 index
positions per table and step, Adagrad.

1. apply_gradients alone over the same queued slices, three arms:

     parent     a checkout of the parent commit (--parent-tree, built there)
     untracked  this tree, no table tracking
     tracked    this tree, every table tracking: one dr_dense_mark_rows over
                the 8 tables in front of the grouped apply

   Every timing runs in a child process of its own (the parent arm is another
   package under the same name); the arms alternate inside each round, and so
   does which goes first.  A child queues the slices, warms up, then times
   `--reps` calls `--inner` times; all of a round's numbers are kept.  Median
   and max - min over every timing of an arm are reported.

2. In this tree: a delta of one step's rows (save_incremental: export of the
   marked rows of table and accumulator, bundle write, marks cleared) against
   the full save of the same tables and slots (save), alternating, for the
   shape above -- where one step touches nearly every row -- and for one table
   of 1 000 000 rows, D = 16, where 65 536 positions touch about 6 % of them.

Host clock around calls that end in a device synchronise.

usage: python tools/dense_ckpt_ab.py --parent-tree DIR [--rounds 5] [--reps 20]
           [--out profiles/dense_ckpt.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES, ROWS, DIM, POSITIONS, LR = 8, 3536, 128, 65536, 0.01
ARMS = ("parent", "untracked", "tracked")
CHILD_LIMIT = 300     # seconds for one child


def _summary(runs, nd=4):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _order(names, r):
    names = list(names)
    names = names[r % len(names):] + names[:r % len(names)]
    if r % 2:
        names.reverse()
    return names


# ---------------------------------------------------------------------------
# children
# ---------------------------------------------------------------------------
def _import(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "deeprec-1_amd"))
    import deeprec_amd as dr
    assert os.path.abspath(dr.__file__).startswith(os.path.abspath(tree) + os.sep), dr.__file__
    dr.load()
    return dr


def _clock(torch, fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def child_apply(args):
    import torch
    dr = _import(args.tree)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    tabs = [dr.DenseTable(torch.randn((ROWS, DIM), generator=g, device=dev) * 0.05)
            for _ in range(TABLES)]
    vals = [torch.randn((POSITIONS, DIM), generator=g, device=dev) * 0.01 for _ in range(TABLES)]
    idxs = [torch.randint(0, ROWS, (POSITIONS,), generator=g, device=dev) for _ in range(TABLES)]
    if args.arm == "tracked":
        for t in tabs:
            t.track_updates()
    opt = dr.AdagradOptimizer(LR, initial_accumulator_value=0.1)

    def step():
        for t, v, i in zip(tabs, vals, idxs):
            t.pending_grads.append(dr.IndexedSlices(v, i))
        opt.apply_gradients(tabs, global_step=1)
    for _ in range(3):
        step()
    runs = [_clock(torch, step, args.reps) for _ in range(args.inner)]
    dr.status_check()
    marked = [t.updated_count() for t in tabs] if args.arm == "tracked" else None
    print("RESULT " + json.dumps({"runs": runs, "marked": marked,
                                  "device": torch.cuda.get_device_name(0)}), flush=True)


def child_delta(args):
    import torch
    dr = _import(args.tree)
    from deeprec_amd import checkpoint as ck
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    out = {}
    for name, ntab, rows, dim in (("8 tables x 3536 rows, D = 128", TABLES, ROWS, DIM),
                                  ("1 table x 1000000 rows, D = 16", 1, 1000000, 16)):
        tabs = {"t%d" % k: dr.DenseTable(torch.randn((rows, dim), generator=g, device=dev) * 0.05,
                                         name="t%d" % k) for k in range(ntab)}
        for t in tabs.values():
            t.track_updates()
        opt = dr.AdagradOptimizer(LR, initial_accumulator_value=0.1)
        state = dict(tabs)
        state.update(opt.checkpoint_variables(tabs))
        vals = torch.randn((POSITIONS, dim), generator=g, device=dev) * 0.01

        def step():
            for t in tabs.values():
                i = torch.randint(0, rows, (POSITIONS,), generator=g, device=dev)
                t.pending_grads.append(dr.IndexedSlices(vals, i))
            opt.apply_gradients(list(tabs.values()), global_step=1)
        res = {"delta ms": [], "full save ms": [], "rows in the delta": [], "delta bytes": [],
               "full bytes": []}
        with tempfile.TemporaryDirectory() as d:
            for r in range(args.rounds + 1):
                step()
                torch.cuda.synchronize()
                res_r = {}
                for what in _order(("delta", "full"), r):
                    if what == "delta":
                        m = sum(t.updated_count() for t in tabs.values())
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        p = ck.save_incremental(os.path.join(d, "delta"), state)
                    else:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        p = ck.save(os.path.join(d, "full"), state)
                    torch.cuda.synchronize()
                    res_r[what] = ((time.perf_counter() - t0) * 1e3,
                                   os.path.getsize(ck.data_path(p)))
                if r == 0:
                    continue                    # warm-up round
                res["delta ms"].append(res_r["delta"][0])
                res["full save ms"].append(res_r["full"][0])
                res["rows in the delta"].append(m)
                res["delta bytes"].append(res_r["delta"][1])
                res["full bytes"].append(res_r["full"][1])
        out[name] = res
        del tabs, state, opt
        torch.cuda.empty_cache()
    dr.status_check()
    print("RESULT " + json.dumps(out), flush=True)


def _run_child(argv):
    """One child under its own time limit; its RESULT line, parsed.  A child
    that fails or runs out of time ends the whole measurement."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True,
                       text=True, timeout=CHILD_LIMIT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("child %s ended with status %d: stopping" % (argv, p.returncode))
    line = [x for x in p.stdout.split("\n") if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_ckpt.json"))
    ap.add_argument("--child", choices=("apply", "delta"))
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.child == "apply":
        return child_apply(args)
    if args.child == "delta":
        return child_delta(args)
    arms = ARMS if args.parent_tree else ARMS[1:]
    trees = {"parent": os.path.abspath(args.parent_tree) if args.parent_tree else None,
             "untracked": ROOT, "tracked": ROOT}
    runs, per_round, marked, device = {a: [] for a in arms}, [], None, None
    common = ["--reps", str(args.reps), "--inner", str(args.inner)]
    for r in range(args.rounds):
        row = {}
        for arm in _order(arms, r):
            got = _run_child(["--child", "apply", "--arm", arm, "--tree", trees[arm]] + common)
            runs[arm] += got["runs"]
            row[arm] = round(statistics.median(got["runs"]), 4)
            marked = got["marked"] or marked
            device = got["device"]
        per_round.append(row)
        print("round %d: %s" % (r, row), flush=True)
    delta = _run_child(["--child", "delta", "--tree", ROOT, "--rounds", str(args.rounds)])
    results = {"apply_gradients alone, %d tables x %d positions, %s ms" % (TABLES, POSITIONS, a):
               _summary(runs[a]) for a in arms}
    for shape, res in delta.items():
        for k, v in res.items():
            results["%s: %s" % (shape, k)] = _summary(v, 3) if k.endswith("ms") else v
    out = {"tables": TABLES, "rows": ROWS, "dim": DIM, "positions": POSITIONS,
           "optimizer": "Adagrad", "rounds": args.rounds, "reps": args.reps, "inner": args.inner,
           "device": device, "parent arm measured": bool(args.parent_tree),
           "median per round": per_round, "marked rows per table (tracked arm)": marked,
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
