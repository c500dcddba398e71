"""Measurement of pooled read-only lookups served from the host-DRAM tier in
place (read_only_lookups(serve_tier=True)).  One pooled
serving call on a tiered EV, against two yardsticks measured in the same run:

  twin        the same call on the untiered twin inside read_only_lookups()
  workaround  what a replica had to do before: promote(keys), the lookup inside
              read_only_lookups(), then demote_to() back to the budget

for two shapes -- 65 536 one-id bags (the fused one-hot route) and 8 192 bags
of 8 ids, combiner mean (the resolve -> pool route) -- and three fractions of
the batch's ids that live in the tier: 0 (the tier is not empty, but the batch
names none of its keys), 1 % and 10 %.

One table (4 M x 128 fp32 by default), a quarter of it demoted.  The cases
alternate inside each of five rounds, and so does which of the three calls
goes first; medians and max - min are reported.  Before anything is timed the
served result is checked bit for bit against the twin's, and after the timed
calls the tier's key count against what it was.  Host clock around calls that
end in a device synchronise; the read-only calls are averaged over --reps
repetitions, the workaround runs once per case and round (it changes both
tiers).

usage: python tools/tier_serve_ab.py [--rows 4000000] [--dim 128] [--rounds 5]
           [--out profiles/tier_serve.json]"""
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
FRACTIONS = (0.0, 0.01, 0.10)


def _summary(runs, nd=3):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _clock(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def _pair(dr, dev, R, D):
    evs = []
    for tiered in (True, False):
        evict = dr.KeyBudgetEvict(R, "lru", steps_to_live=10**9) if tiered \
            else dr.GlobalStepEvict(10**9)
        opt = dr.EmbeddingVariableOption(
            evict_option=evict,
            storage_option=dr.StorageOption(dr.StorageType.HBM_DRAM) if tiered else None)
        ev = dr.EmbeddingVariable("serve_ab_%d" % tiered, D, 0.0, ev_option=opt, device=dev,
                                  capacity=R)
        ev.insert_synthetic(0, R, seed=77)
        evs.append(ev)
    return evs


def _batch(dr, dev, g, shape, frac, tier_keys, resident):
    """A SparseTensor of `shape` whose ids are, to the fraction `frac`, keys of
    the tier, the others resident in HBM; shuffled, duplicates possible."""
    nnz = ONEHOT if shape == "onehot" else BAGS * BAG_LEN
    n_t = int(round(nnz * frac))
    pick = lambda src, n: src[torch.randint(0, src.numel(), (n,), generator=g, device=dev)]
    ids = torch.cat([pick(tier_keys, n_t), pick(resident, nnz - n_t)])
    ids = ids[torch.randperm(nnz, generator=g, device=dev)].contiguous()
    if shape == "onehot":
        ind = torch.stack([torch.arange(nnz, device=dev), torch.zeros(nnz, dtype=torch.int64,
                                                                     device=dev)], 1)
        return dr.SparseTensor(ind, ids, (nnz, 1)), "sum", n_t
    ar = torch.arange(nnz, device=dev)
    ind = torch.stack([ar // BAG_LEN, ar % BAG_LEN], 1)
    return dr.SparseTensor(ind, ids, (BAGS, BAG_LEN)), "mean", n_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4000000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tier_serve.json"))
    args = ap.parse_args()
    import deeprec_amd as dr
    dev = torch.device("cuda", 0)
    R, D = args.rows, args.dim
    a, b = _pair(dr, dev, R, D)
    budget = R - R // 4
    t_demote, n = _clock(lambda: a.demote_to(budget))
    assert n == R // 4 and a.tier_count() == R // 4
    print("demoted %d keys in %.1f ms" % (n, t_demote), flush=True)
    g = torch.Generator(device=dev)
    res, info = {}, {}

    def lookup(ev, sp, comb, serve):
        with dr.read_only_lookups(serve_tier=serve):
            return dr.embedding_lookup_sparse(ev, sp, combiner=comb)

    def workaround(sp, comb):
        a.promote(sp.values)
        out = lookup(a, sp, comb, False)
        a.demote_to(budget)
        return out

    cases = [(s, f) for s in ("onehot", "bags") for f in FRACTIONS]
    for r in range(args.rounds):
        g.manual_seed(101 + r)
        order = cases[r % len(cases):] + cases[:r % len(cases)]
        for ci, (shape, frac) in enumerate(order):
            with a._lock:
                tk = torch.from_numpy(a._tier_export(columns=())[0]).to(dev)
            mask = torch.ones(R, dtype=torch.bool, device=dev)
            mask[tk] = False
            resident = torch.nonzero(mask).reshape(-1)
            sp, comb, n_t = _batch(dr, dev, g, shape, frac, tk, resident)
            tag = "%s, %g %% in the tier" % (shape, frac * 100)
            info[tag] = {"nnz": sp.values.numel(), "tier ids": n_t}
            # checked before it is timed: the served result is the twin's, bit for bit
            want = lookup(b, sp, comb, False)
            got = lookup(a, sp, comb, True)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), tag
            assert a.tier_count() == R // 4
            runs = {"twin": lambda: lookup(b, sp, comb, False),
                    "serve_tier": lambda: lookup(a, sp, comb, True)}
            names = ["twin", "serve_tier"]
            if (r + ci) % 2:
                names.reverse()
            for name in names:
                t, _ = _clock(runs[name], reps=args.reps)
                res.setdefault("%s: %s ms" % (tag, name), []).append(t)
            t, out = _clock(lambda: workaround(sp, comb))
            res.setdefault("%s: promote + lookup + demote_to ms" % tag, []).append(t)
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), tag
            assert a.tier_count() == R // 4 and int(a.total_count()[0]) == budget
        print("round %d done" % r, flush=True)
    out = {"rows": R, "dim": D, "rounds": args.rounds, "reps": args.reps,
           "tier keys": R // 4, "demote_to ms": round(t_demote, 1),
           "device": torch.cuda.get_device_name(0), "cases": info,
           "results": {k: _summary(v) for k, v in sorted(res.items())}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["results"], indent=1, sort_keys=True))
    dr.status_check()


if __name__ == "__main__":
    main()
