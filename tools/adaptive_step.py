"""Training step of adaptive-embedding features against plain EV features:
forward (embedding_lookup_sparse_multi) + backward + apply_gradients (Adagrad)
of --features one-hot features at batch B, dim D, ids uniform over --ids
possible ids.  Arms:

  ev            plain EmbeddingVariable features (every id gets a private row)
  adaptive_P    AdaptiveEmbeddingVariable features, P % of the ids masked into
                the EV (the mask is a function of the id), the others training a
                hash table of --bucket rows; P = 10, 50, 100

Every arm sees the same ids.  Per arm and repeat: fresh variables, --warmup
untimed steps, then --steps steps timed one by one with device events.  The
arms alternate inside a repeat, so drift of the machine hits all of them.
Reported per arm: the median, p10 / p90 and extremes of the step time over
all repeats, each repeat's median (the spread between runs of the same code),
and after the last step of a repeat the EV keys and the device memory the
arm's variables and optimizer slots hold (hipMemGetInfo before / after, the
torch cache emptied).  Prints one JSON line; --out also writes it to a file.

  python tools/adaptive_step.py [--batch 65536] [--dim 128] [--steps 50] [--out FILE]
"""
import argparse
import datetime
import gc
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))


def id_mask(ids, pct):
    """1 for pct % of the ids: a multiplicative hash of the id, so every
    position of an id agrees."""
    if pct >= 100:
        return torch.ones_like(ids)
    h = (ids * 2654435761) >> 7
    return (torch.remainder(h, 100) < pct).to(torch.int64)


def used_bytes(dev):
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(dev)
    return total - free


def run_arm(dr, arm, args, dev, ids, grad, ind):
    import deeprec_amd.kv_variable_ops as kv
    T, D, B = args.features, args.dim, args.batch
    pct = None if arm == "ev" else int(arm.split("_")[1])
    kv.reset_registry()
    dr.flush_releases()
    base = used_bytes(dev)
    if pct is None:
        vs = [dr.get_embedding_variable("as_ev%d" % t, D, initializer=0.0, device=dev)
              for t in range(T)]
    else:
        vs = [dr.get_adaptive_embedding_variable(
            "as_ad%d" % t, D, args.bucket,
            initializer=lambda s: torch.randn(s, generator=torch.Generator().manual_seed(7)) * 0.01,
            device=dev) for t in range(T)]
    opt = dr.AdagradOptimizer(0.05, initial_accumulator_value=0.1)
    times = []
    n_steps = args.warmup + args.steps
    for step in range(n_steps):
        sps = [dr.SparseTensor(ind, ids[step, t], (B, 1)) for t in range(T)]
        masks = None if pct is None else [id_mask(ids[step, t], pct) for t in range(T)]
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = dr.embedding_lookup_sparse_multi(vs, sps, combiner="sum", adaptive_masks=masks)
        out.backward(grad)
        opt.apply_gradients(vs, global_step=step)
        e1.record()
        torch.cuda.synchronize(dev)
        if step >= args.warmup:
            times.append(e0.elapsed_time(e1))
    dr.status_check()
    evs = vs if pct is None else [v.ev for v in vs]
    keys = sum(int(e.total_count()[0]) for e in evs)
    del out, sps, masks
    held = used_bytes(dev) - base
    res = dict(times_ms=times, ev_keys=keys, hbm_bytes=int(held),
               hash_table_bytes=0 if pct is None else T * args.bucket * D * 4)
    del vs, evs, opt
    kv.reset_registry()
    gc.collect()
    dr.flush_releases()
    return res


def pctl(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=4)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--ids", type=int, default=12_500_000)
    ap.add_argument("--bucket", type=int, default=100_003)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--arms", default="ev,adaptive_10,adaptive_50,adaptive_100")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded as is (default: git rev-parse)")
    args = ap.parse_args()
    import deeprec_amd as dr
    dr.load()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_step.py measures on the GPU; none is visible")
    dr.set_validate(False)
    dev = torch.device("cuda", 0)
    T, D, B = args.features, args.dim, args.batch
    gen = torch.Generator().manual_seed(2024)
    n_steps = args.warmup + args.steps
    ids = torch.randint(0, args.ids, (n_steps, T, B), generator=gen, dtype=torch.int64).to(dev)
    grad = (torch.randn((B, T * D), generator=gen) * 0.01).to(dev)
    ind = torch.stack([torch.arange(B), torch.zeros(B, dtype=torch.int64)], 1).to(dev)
    arms = args.arms.split(",")
    runs = {a: [] for a in arms}
    for _ in range(args.repeats):
        for a in arms:
            runs[a].append(run_arm(dr, a, args, dev, ids, grad, ind))
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                             stderr=subprocess.DEVNULL, text=True).strip()
        except Exception:
            commit = None
    res = dict(tool="adaptive_step", date=datetime.date.today().isoformat(),
               device=torch.cuda.get_device_name(dev), commit=commit, features=T,
               batch=B, dim=D, possible_ids=args.ids, bucket_size=args.bucket,
               steps=args.steps, warmup=args.warmup, repeats=args.repeats, optimizer="adagrad",
               distinct_ids_per_feature=int(torch.unique(ids[:, 0]).numel()), arms={})
    for a in arms:
        allt = [x for r in runs[a] for x in r["times_ms"]]
        res["arms"][a] = dict(
            ms_per_step_median=round(statistics.median(allt), 4),
            ms_per_step_p10=round(pctl(allt, 0.1), 4), ms_per_step_p90=round(pctl(allt, 0.9), 4),
            ms_per_step_min=round(min(allt), 4), ms_per_step_max=round(max(allt), 4),
            repeat_medians_ms=[round(statistics.median(r["times_ms"]), 4) for r in runs[a]],
            ev_keys=runs[a][-1]["ev_keys"], hbm_bytes=runs[a][-1]["hbm_bytes"],
            hbm_bytes_per_repeat=[r["hbm_bytes"] for r in runs[a]],
            hash_table_bytes=runs[a][-1]["hash_table_bytes"],
            # the per-key default block the split writes and the resolve reads
            defaults_bytes_per_step=0 if a == "ev" else T * B * D * 4 * int(a.split("_")[1]) // 100)
    if "ev" in res["arms"]:
        base = res["arms"]["ev"]["ms_per_step_median"]
        for a in arms:
            res["arms"][a]["vs_ev"] = round(res["arms"][a]["ms_per_step_median"] / base, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
