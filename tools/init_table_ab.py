"""Measurement of the EV init table, by section 14's
method: the cases alternate inside each of five rounds, fresh tables per
round, medians and max - min are reported.

Workload: 26 EVs x 1 M keys x dim 128 fp32, one-hot batches of 65 536 ids per
table, one training step = embedding_lookup_sparse_multi forward + backward +
GradientDescentOptimizer.apply_gradients, eager (no graph), host clock around
steps that end in a device synchronise.

  a  constant initializer (existing code: the yardstick)
  b  with_init_option(InitializerOption(normal, default_value_dim=4096))
  c  a callable initializer without init_option (existing code: the per-call
     draw, prepared feature by feature)

Each case is timed in steady state (every id known) and with 10 % new keys
per step.  Before anything is timed the tables are checked: a sample of the
populated keys and a batch of fresh keys through the fused one-hot lookup read
table[key % K] on (b) and the constant row on (a).

usage: python tools/init_table_ab.py [--rows 1000000] [--tables 26] [--dim 128]
           [--batch 65536] [--steps 10] [--warmup 3] [--rounds 5]
           [--out profiles/init_table.json]"""
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

K = 4096
CONST = 0.125


def _summary(runs, nd=4):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "min": round(min(runs), nd), "max": round(max(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _normal(seed):
    def init(shape):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(shape, generator=g) * 0.05
    return init


def _tables(dr, case, tag, a, dev):
    evs = []
    for t in range(a.tables):
        name = "ita_%s_%s_%d" % (tag, case, t)
        cap = a.rows + (a.steps + a.warmup + 2) * a.batch
        if case == "a":
            ev = dr.EmbeddingVariable(name, a.dim, CONST, device=dev, capacity=cap)
        elif case == "b":
            o = dr.EmbeddingVariableOption().with_init_option(dr.InitializerOption(_normal(t), K))
            ev = dr.EmbeddingVariable(name, a.dim, None, ev_option=o, device=dev, capacity=cap)
        else:
            ev = dr.EmbeddingVariable(name, a.dim, lambda s: torch.randn(s, device=dev) * 0.05,
                                      device=dev, capacity=cap)
        evs.append(ev)
    # populate keys 0 .. rows-1 through the lookup itself
    with torch.no_grad():
        for lo in range(0, a.rows, a.batch):
            keys = torch.arange(lo, min(lo + a.batch, a.rows), dtype=torch.int64, device=dev)
            for ev in evs:
                ev.sparse_read(keys)
    return evs


def _onehot(dr, ids, dev):
    B = ids.shape[1]
    ind = torch.stack([torch.arange(B, device=dev), torch.zeros(B, dtype=torch.int64,
                                                                device=dev)], 1)
    return [dr.SparseTensor(ind, ids[t], (B, 1)) for t in range(ids.shape[0])]


def _expect(ev, case, keys):
    if case == "b":
        return ev.init_table[torch.remainder(keys, K)]       # floor mod, as Python's %
    return torch.full((keys.numel(), ev.dim), CONST, device=keys.device)


def _check(dr, evs, case, a, dev, rng):
    """Populated and fresh keys read table[key % K] (b) / the constant (a)."""
    if case == "c":
        return
    sample = torch.randint(0, a.rows, (4096,), generator=rng).to(dev)
    for ev in evs:
        if not torch.equal(ev.sparse_read(sample), _expect(ev, case, sample)):
            raise AssertionError("%s: populated keys differ from their initial rows" % ev.name)
    fresh = (torch.randint(0, 1 << 40, (len(evs), a.batch), generator=rng) + (1 << 50)).to(dev)
    fresh[:, :4] = torch.tensor([-1, -2, -(1 << 63), (1 << 63) - 1], device=dev)
    with torch.no_grad():
        out = dr.embedding_lookup_sparse_multi(evs, _onehot(dr, fresh, dev), combiner="sum")
    out = out.reshape(a.batch, len(evs), a.dim)
    for t, ev in enumerate(evs):
        if not torch.equal(out[:, t, :], _expect(ev, case, fresh[t])):
            raise AssertionError("%s: fresh keys differ from their initial rows" % ev.name)
    dr.status_check()


def _time(dr, evs, batches, grads, a):
    opt = dr.GradientDescentOptimizer(0.01)

    def step(i):
        out = dr.embedding_lookup_sparse_multi(evs, batches[i], combiner="sum")
        out.backward(grads)
        opt.apply_gradients(evs, global_step=i + 1)

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.warmup, a.warmup + a.steps):
        step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / a.steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--tables", type=int, default=26)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--batch", type=int, default=65536)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_table.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("init_table_ab.py measures on the MI355X: no GPU found")
    import deeprec_amd as dr
    dr.load()
    dev = torch.device("cuda", 0)
    rng = torch.Generator().manual_seed(18)
    n = a.warmup + a.steps
    T, B = a.tables, a.batch
    grads = torch.randn((B, T * a.dim), generator=rng).to(dev)
    res = {c + "_" + m: [] for c in "abc" for m in ("steady", "new10")}
    for rnd in range(a.rounds):
        steady, new10 = [], []
        for i in range(n):
            ids = torch.randint(0, a.rows, (T, B), generator=rng)
            steady.append(_onehot(dr, ids.to(dev), dev))
            ids = torch.randint(0, a.rows, (T, B), generator=rng)
            new = torch.rand((T, B), generator=rng) < 0.1
            fresh = a.rows + (rnd * n + i) * B + torch.arange(B).expand(T, B)   # never seen before
            new10.append(_onehot(dr, torch.where(new, fresh, ids).to(dev), dev))
        tables = {}
        for case in "abc":
            tables[case] = _tables(dr, case, "r%d" % rnd, a, dev)
            _check(dr, tables[case], case, a, dev, rng)
        for mode, batches in (("steady", steady), ("new10", new10)):
            for case in ("abc" if rnd % 2 == 0 else "cba"):       # alternated inside the round
                res[case + "_" + mode].append(_time(dr, tables[case], batches, grads, a))
        dr.status_check()
        del tables
        dr.flush_releases()
        torch.cuda.empty_cache()
        print("round %d: %s" % (rnd, {k: round(v[-1], 3) for k, v in res.items()}), flush=True)
    out = {"workload": {"tables": T, "rows": a.rows, "dim": a.dim, "batch": B, "K": K,
                        "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                        "step": "embedding_lookup_sparse_multi + backward + SGD apply, eager",
                        "device": torch.cuda.get_device_name(0)},
           "ms_per_step": {k: _summary(v) for k, v in res.items()}}
    ms = out["ms_per_step"]
    out["b_steady_median_inside_a_min_max"] = \
        ms["a_steady"]["min"] <= ms["b_steady"]["median"] <= ms["a_steady"]["max"]
    out["c_over_b"] = {m: round(ms["c_" + m]["median"] / ms["b_" + m]["median"], 2)
                       for m in ("steady", "new10")}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
