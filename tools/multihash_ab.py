"""Measurement of the fused MultiHashVariable ("Q-R") lookup (DESIGN section
20): embedding_lookup_sparse_multi over T multi-hash features, against two
yardsticks measured in the same run:

  materialised  the same call over DenseTables that hold the combined rows
                (Q*Q x dim each): what the trick replaces
  composed      what a user could write before from public ops: two
                embedding_lookups (of Q by q, of R by r), the torch op, the
                pooled reduce (ops.sparse_segment_*), torch.cat over features

Shapes: one-hot B = 65 536 with sum, and 8 192 bags of 8 with mean; D = 128,
Q = R = 3 536; add, mul and concat (64 + 64).  T = 26, or the largest T whose
materialised tables fit a share of the free HBM (recorded).  The variants
alternate inside each of five rounds, and so does which goes first; medians
and max - min are reported.  Every result is checked bit for bit against the
materialised lookup before anything is timed.  Host clock around calls that
end in a device synchronise, averaged over --reps repetitions.

One training step (forward, backward, Adagrad on the tables) is timed the same
way for the fused path, the materialised tables and a plain-torch composition
(the engine's unpooled lookups carry no gradient, so that is what a user could
write), over --train-tables features: the materialised tables need a second
copy for their accumulators.

Also reported: output bytes per second of the fused forward (B x T x dim x 4
over the call time -- an end-to-end figure with launch overheads inside, not a
kernel's share of peak), next to the cache-resident gather rates a kernel can
reach on this chip.

usage: python tools/multihash_ab.py [--tables 26] [--rounds 5] [--reps 20]
           [--out profiles/multihash.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))

import torch  # noqa: E402

ONEHOT = 65536
BAGS, BAG_LEN = 8192, 8
QR = 3536
DIM = 128
OPS = (("add", DIM, DIM), ("mul", DIM, DIM), ("concat", DIM // 2, DIM // 2))
# cache-resident gather rates of the chip, TB/s (published guide figures, not
# measured here): rows of a table shared in one XCD's L2; uniformly random rows
# of a 38 MB table (Infinity Cache); whole rows from HBM
GUIDE_TBS = {"table shared in L2": [16.8, 18.8], "38 MB table, random rows": 8.6,
             "whole rows from HBM": [5.5, 5.8]}


def _summary(runs, nd=4):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _clock(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _batch(dr, dev, g, shape, T):
    nnz = ONEHOT if shape == "onehot" else BAGS * BAG_LEN
    ids = torch.randint(0, QR * QR, (T, nnz), generator=g, device=dev)
    ar = torch.arange(nnz, device=dev)
    if shape == "onehot":
        ind = torch.stack([ar, torch.zeros_like(ar)], 1)
        return [dr.SparseTensor(ind, ids[t], (nnz, 1)) for t in range(T)], "sum", nnz
    ind = torch.stack([ar // BAG_LEN, ar % BAG_LEN], 1)
    return [dr.SparseTensor(ind, ids[t], (BAGS, BAG_LEN)) for t in range(T)], "mean", BAGS


def _composed(dr, ops, v, sp, comb, onehot, seg, pos):
    qt, rt = v.val_list
    ids = sp.values
    a = dr.embedding_lookup(qt, ids // qt.weight.shape[0])
    b = dr.embedding_lookup(rt, ids % rt.weight.shape[0])
    rows = a + b if v.operation == "add" else a * b if v.operation == "mul" else \
        torch.cat([a, b], 1)
    if onehot:
        return rows
    red = {"sum": ops.sparse_segment_sum, "mean": ops.sparse_segment_mean,
           "sqrtn": ops.sparse_segment_sqrt_n}[comb]
    return red(rows, pos, seg, num_segments=sp.dense_shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=26)
    ap.add_argument("--train-tables", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hbm-share", type=float, default=0.6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multihash.json"))
    args = ap.parse_args()
    import deeprec_amd as dr
    from deeprec_amd import ops
    dev = torch.device("cuda", 0)
    free, total = torch.cuda.mem_get_info(dev)
    mat_bytes = QR * QR * DIM * 4
    T = max(1, min(args.tables, int(free * args.hbm_share) // mat_bytes))
    Tt = max(1, min(args.train_tables, T))
    print("T = %d (asked %d; %.1f GB free, %.2f GB per materialised table)"
          % (T, args.tables, free / 1e9, mat_bytes / 1e9), flush=True)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    res, info = {}, {}
    all_ids = torch.arange(QR * QR, device=dev)
    for op, dq, dr_ in OPS:
        vs, mats = [], []
        for t in range(T):
            init = [torch.randn((QR, d), generator=g, device=dev) * 0.05 for d in (dq, dr_)]
            v = dr.get_multihash_variable("ab_%s_%d" % (op, t), [[QR, dq], [QR, dr_]],
                                          operation=op, initializer=init, device=dev)
            vs.append(v)
            mats.append(dr.DenseTable(dr.embedding_lookup(v, all_ids)))
        # every forward case first: the training steps change the tables, and a
        # fused / materialised pair then no longer holds the same rows
        batches = {shape: _batch(dr, dev, g, shape, T) for shape in ("onehot", "bags")}
        for shape, (sps, comb, B) in batches.items():
            onehot = shape == "onehot"
            nnz = sps[0].values.numel()
            seg = sps[0].indices[:, 0].to(torch.int32).contiguous()
            pos = torch.arange(nnz, dtype=torch.int32, device=dev)
            runs = {
                "fused": lambda: dr.embedding_lookup_sparse_multi(vs, sps, combiner=comb),
                "materialised": lambda: dr.embedding_lookup_sparse_multi(mats, sps,
                                                                         combiner=comb),
                "composed": lambda: torch.cat(
                    [_composed(dr, ops, v, sp, comb, onehot, seg, pos)
                     for v, sp in zip(vs, sps)], 1),
            }
            tag = "%s %s" % (shape, op)
            with torch.no_grad():
                want = runs["materialised"]()
                for name in ("fused", "composed"):   # checked before anything is timed
                    assert _same(runs[name](), want), (tag, name)
                del want
                for r in range(args.rounds):
                    names = list(runs)
                    names = names[r % 3:] + names[:r % 3]
                    if r % 2:
                        names.reverse()
                    for name in names:
                        t, _ = _clock(runs[name], reps=args.reps)
                        res.setdefault("%s: %s ms" % (tag, name), []).append(t)
            info[tag] = {"batch": B, "nnz per feature": nnz, "combiner": comb,
                         "output bytes": B * T * DIM * 4}
            print("%s forward done" % tag, flush=True)
        # one training step over the first Tt features
        for shape, (sps, comb, B) in batches.items():
            onehot = shape == "onehot"
            tag = "%s %s" % (shape, op)
            vt, mt, st = vs[:Tt], mats[:Tt], sps[:Tt]
            gout = torch.randn((B, Tt * DIM), generator=g, device=dev)
            o1, o2 = dr.AdagradOptimizer(0.01), dr.AdagradOptimizer(0.01)
            pq = [[torch.nn.Parameter(t.weight.clone()) for t in v.val_list] for v in vt]
            o3 = torch.optim.Adagrad([p for pair in pq for p in pair], lr=0.01,
                                     initial_accumulator_value=0.1)

            def step_engine(params, opt):
                out = dr.embedding_lookup_sparse_multi(params, st, combiner=comb)
                out.backward(gout)
                opt.apply_gradients(params, global_step=1)

            def step_torch():
                outs = []
                for (qp, rp), sp in zip(pq, st):
                    a, b = qp[sp.values // QR], rp[sp.values % QR]
                    rows = a + b if op == "add" else a * b if op == "mul" else \
                        torch.cat([a, b], 1)
                    outs.append(rows if onehot else rows.view(B, BAG_LEN, -1).mean(1))
                o3.zero_grad(set_to_none=True)
                torch.cat(outs, 1).backward(gout)
                o3.step()

            steps = {"fused": lambda: step_engine(vt, o1),
                     "materialised": lambda: step_engine(mt, o2),
                     "composed (plain torch)": step_torch}
            for name in steps:
                steps[name]()                      # warm-up (slot allocation, code objects)
            for r in range(args.rounds):
                names = list(steps)
                names = names[r % 3:] + names[:r % 3]
                if r % 2:
                    names.reverse()
                for name in names:
                    t, _ = _clock(steps[name], reps=max(1, args.reps // 4))
                    res.setdefault("%s: train step, %d features, %s ms" % (tag, Tt, name),
                                   []).append(t)
            del o2, o3, pq
            print("%s done" % tag, flush=True)
        del vs, mats
        torch.cuda.empty_cache()
    results = {k: _summary(v) for k, v in sorted(res.items())}
    rates = {}
    for tag, i in info.items():
        ms = results["%s: fused ms" % tag]["median"]
        rates[tag] = round(i["output bytes"] / (ms * 1e-3) / 1e12, 3)
    out = {"tables": T, "tables asked": args.tables, "train tables": Tt, "dim": DIM,
           "q rows": QR, "r rows": QR, "rounds": args.rounds, "reps": args.reps,
           "free HBM at start GB": round(free / 1e9, 1),
           "materialised table GB": round(mat_bytes / 1e9, 2),
           "device": torch.cuda.get_device_name(0), "cases": info, "results": results,
           "fused forward, output TB/s (call time, launch overheads included)": rates,
           "guide gather rates TB/s (not measured here)": GUIDE_TBS}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"results": results, "rates": rates}, indent=1, sort_keys=True))
    dr.status_check()


if __name__ == "__main__":
    main()
