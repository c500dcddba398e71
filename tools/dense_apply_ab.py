"""Measurement of the grouped dense-table apply on section
20's training-step shape: 4 MultiHashVariable features, Q = R = 3 536,
D = 128, one-hot B = 65 536 and 8 192 bags of 8; add / mul / concat; Adagrad.
Three arms, measured in the same run:

  native       the tree as it is: dr_dense_apply_grouped, one call for the
               eight tables, no host read
  torch        the same tree with training._NATIVE_DENSE off (what
               DR_DENSE_APPLY=torch selects, the behaviour before the native
               apply): unique + unsorted_segment_sum + torch indexing, three
               host reads per table
  plain torch  nn.Parameter tables, torch indexing, torch.optim.Adagrad

Timed: the whole step (forward, backward, optimizer) for all three, and the
optimizer step alone (apply_gradients over the queued slices) for the two
engine arms.  The arms alternate inside each of five rounds, and so does which
goes first; 20 calls per timing; median and max - min are reported.  Before
anything is timed one step of every arm is checked from equal tables: native
bit for bit against the CPU oracle's unique + unsorted_segment_sum + Adagrad
over the queued slices (tests/multihash_ref.py), torch against the same to
rtol 1e-5 / atol 1e-7 (torch.rsqrt is not 1.0f / sqrtf), plain torch to rtol 1e-3 (its
dense gradient sums in another order).  Host clock around calls that end in a
device synchronise.

Last, the cost of long runs (one lane group walks a run): one table, 65 536
positions, apply_gradients alone, for uniformly random rows, 128 runs of 512
and every position on one row; the two engine arms, the same rounds.

--opt adam | ftrl | adagrad_decay | all measures the
optimizers of dr_dense_apply_grouped_ex instead, with the same method:
apply_gradients alone over 8 DenseTables of [3 536, 128] with 65 536 positions
each (section 21's shape), native against the torch arm, after one step of
both arms from equal tables is checked against tests/dense_opt_ref.py (native
bit for bit; FTRL here has lr_power -0.5).  With adam also one table of
[2^20, 128] with 65 536 positions, where the sweep over the unnamed rows
dominates; --sweep-only N runs just N native steps of that (for a kernel
trace of its own) and prints the bytes the sweep moves per call.

usage: python tools/dense_apply_ab.py [--features 4] [--rounds 5] [--reps 20]
           [--opt adagrad] [--sweep-only 0] [--out profiles/dense_apply.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

ONEHOT = 65536
BAGS, BAG_LEN = 8192, 8
QR = 3536
DIM = 128
LR = 0.01
OPS = (("add", DIM, DIM), ("mul", DIM, DIM), ("concat", DIM // 2, DIM // 2))
ARMS = ("native", "torch", "plain torch")


def _summary(runs, nd=4):
    return {"runs": [round(x, nd) for x in runs], "median": round(statistics.median(runs), nd),
            "spread": round(max(runs) - min(runs), nd)}


def _clock(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _batch(dr, dev, g, shape, T):
    nnz = ONEHOT if shape == "onehot" else BAGS * BAG_LEN
    ids = torch.randint(0, QR * QR, (T, nnz), generator=g, device=dev)
    ar = torch.arange(nnz, device=dev)
    if shape == "onehot":
        ind = torch.stack([ar, torch.zeros_like(ar)], 1)
        return [dr.SparseTensor(ind, ids[t], (nnz, 1)) for t in range(T)], "sum", nnz
    ind = torch.stack([ar // BAG_LEN, ar % BAG_LEN], 1)
    return [dr.SparseTensor(ind, ids[t], (BAGS, BAG_LEN)) for t in range(T)], "mean", BAGS


def _order(names, r):
    names = list(names)
    names = names[r % len(names):] + names[:r % len(names)]
    if r % 2:
        names.reverse()
    return names


BIG_ROWS = 1 << 20
EX_OPTS = ("adam", "ftrl", "adagrad_decay")


def _ex_optimizer(dr, name):
    if name == "adam":
        return dr.AdamOptimizer(LR)
    if name == "ftrl":
        return dr.FtrlOptimizer(LR, l1_regularization_strength=0.001,
                                l2_regularization_strength=0.001)
    return dr.AdagradDecayOptimizer(LR, global_step=0, accumulator_decay_step=1)


def _ex_reference(orc, name, w, idx, val):
    """One first step of a fresh optimizer of _ex_optimizer on table w."""
    import dense_opt_ref as ref
    if name == "adam":
        ref.adam(orc, w, np.zeros_like(w), np.zeros_like(w), idx, val, LR, 0.9, 0.999, 1e-8,
                 0.9, 0.999)
    elif name == "ftrl":
        ref.ftrl(orc, w, np.full_like(w, 0.1), np.zeros_like(w), idx, val, LR, 0.001, 0.001,
                 -0.5, 0.0)
    else:
        ref.adagrad_decay(orc, w, np.full_like(w, 0.1), np.zeros(w.shape[0], np.int64), idx, val,
                          LR, 1, 0.9, 0.1, 1)
    return w


def _ex_arms(dr, training, name, tables, idxs, vals):
    """{arm: call} -- one apply_gradients over copies of `tables`, each with
    its slice queued again."""
    calls, state = {}, {}
    for arm in ARMS[:2]:
        tabs = [dr.DenseTable(t.clone()) for t in tables]
        opt = _ex_optimizer(dr, name)
        state[arm] = tabs

        def call(arm=arm, tabs=tabs, opt=opt):
            for tab, i, v in zip(tabs, idxs, vals):
                tab.pending_grads.append(dr.IndexedSlices(v, i))
            training._NATIVE_DENSE = arm == "native"
            try:
                opt.apply_gradients(tabs)
            finally:
                training._NATIVE_DENSE = True
        calls[arm] = call
    return calls, state


def main_ex(args):
    import deeprec_amd as dr
    from deeprec_amd import training
    from oracle import oracle as orc
    orc.build()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    names = EX_OPTS if args.opt == "all" else (args.opt,)
    T = 2 * args.features
    res, checks = {}, {}
    if not args.sweep_only:
        tables = [torch.randn((QR, DIM), generator=g, device=dev) * 0.05 for _ in range(T)]
        idxs = [torch.randint(0, QR, (ONEHOT,), generator=g, device=dev) for _ in range(T)]
        vals = [torch.randn((ONEHOT, DIM), generator=g, device=dev) * 0.01 for _ in range(T)]
        for name in names:
            calls, state = _ex_arms(dr, training, name, tables, idxs, vals)
            for arm in calls:
                calls[arm]()                       # the checked step (and the warm-up)
            dr.status_check()
            diff = 0
            for k in range(T):
                want = _ex_reference(orc, name, tables[k].cpu().numpy().copy(),
                                     idxs[k].cpu().numpy(), vals[k].cpu().numpy())
                got = state["native"][k].weight.cpu().numpy()
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, k)
                got_t = state["torch"][k].weight.cpu().numpy()
                np.testing.assert_allclose(got_t, want, rtol=1e-5, atol=1e-6)
                diff += int((got_t.view(np.int32) != want.view(np.int32)).sum())
            checks[name] = {"native == reference (bits)": True,
                            "torch arm elements differing from the reference in bits": diff,
                            "elements": T * QR * DIM}
            for r in range(args.rounds):
                for arm in _order(ARMS[:2], r):
                    res.setdefault("%s: apply_gradients alone, %d tables x %d positions, %s ms"
                                   % (name, T, ONEHOT, arm), []).append(
                        _clock(calls[arm], args.reps))
            del calls, state
            torch.cuda.empty_cache()
            print("%s done" % name, flush=True)
    extra = {}
    if "adam" in names:
        table = torch.randn((BIG_ROWS, DIM), generator=g, device=dev) * 0.05
        idx = torch.randint(0, BIG_ROWS, (ONEHOT,), generator=g, device=dev)
        val = torch.randn((ONEHOT, DIM), generator=g, device=dev) * 0.01
        unnamed = BIG_ROWS - int(torch.unique(idx).numel())
        # what the sweep moves: w, m, v of every row read, of every unnamed row written
        extra = {"big table rows": BIG_ROWS, "unnamed rows": unnamed,
                 "sweep bytes per call": (3 * BIG_ROWS + 3 * unnamed) * DIM * 4,
                 "six full row passes bytes": 6 * BIG_ROWS * DIM * 4}
        calls, _ = _ex_arms(dr, training, "adam", [table], [idx], [val])
        del table
        if args.sweep_only:
            for _ in range(args.sweep_only + 2):
                calls["native"]()
            torch.cuda.synchronize()
            dr.status_check()
            print(json.dumps(extra, sort_keys=True))
            return
        for arm in calls:
            calls[arm]()                           # warm-up
        for r in range(args.rounds):
            for arm in _order(ARMS[:2], r):
                res.setdefault("adam: apply_gradients alone, 1 table of %d rows x %d positions, "
                               "%s ms" % (BIG_ROWS, ONEHOT, arm), []).append(
                    _clock(calls[arm], max(1, args.reps // 4)))
    results = {k: _summary(v) for k, v in sorted(res.items())}
    out = {"tables": T, "dim": DIM, "rows": QR, "positions": ONEHOT, "rounds": args.rounds,
           "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "checked before timing": checks, "results": results, "adam sweep case": extra}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"results": results, "checks": checks, "adam sweep case": extra}, indent=1,
                     sort_keys=True))
    dr.status_check()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--opt", default="adagrad", choices=("adagrad", "all") + EX_OPTS)
    ap.add_argument("--sweep-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "dense_apply.json" if args.opt == "adagrad"
                                else "dense_apply_opts.json")
    if args.opt != "adagrad":
        return main_ex(args)
    import deeprec_amd as dr
    from deeprec_amd import training
    from oracle import oracle as orc
    import multihash_ref as ref
    orc.build()
    dev = torch.device("cuda", 0)
    T = args.features
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    res, checks = {}, {}

    def engine_arm(native):
        def run(fn):
            training._NATIVE_DENSE = native
            try:
                fn()
            finally:
                training._NATIVE_DENSE = True
        return run

    for op, dq, dr_ in OPS:
        init = [[torch.randn((QR, d), generator=g, device=dev) * 0.05 for d in (dq, dr_)]
                for _ in range(T)]

        def variables(tag):
            return [dr.get_multihash_variable("ab_%s_%s_%d" % (op, tag, t), [[QR, dq], [QR, dr_]],
                                              operation=op,
                                              initializer=[x.clone() for x in init[t]], device=dev)
                    for t in range(T)]
        for shape in ("onehot", "bags"):
            sps, comb, B = _batch(dr, dev, g, shape, T)
            onehot = shape == "onehot"
            tag = "%s %s" % (shape, op)
            gout = torch.randn((B, T * DIM), generator=g, device=dev)
            vs = {"native": variables("n" + shape), "torch": variables("t" + shape)}
            opts = {a: dr.AdagradOptimizer(LR, initial_accumulator_value=0.1) for a in vs}
            run = {"native": engine_arm(True), "torch": engine_arm(False)}
            pq = [[torch.nn.Parameter(x.clone()) for x in pair] for pair in init]
            o3 = torch.optim.Adagrad([p for pair in pq for p in pair], lr=LR,
                                     initial_accumulator_value=0.1)

            def forward_backward(arm):
                out = dr.embedding_lookup_sparse_multi(vs[arm], sps, combiner=comb)
                out.backward(gout)

            def apply(arm):
                run[arm](lambda: opts[arm].apply_gradients(vs[arm], global_step=1))

            def step_engine(arm):
                forward_backward(arm)
                apply(arm)

            def step_torch():
                outs = []
                for (qp, rp), sp in zip(pq, sps):
                    a, b = qp[sp.values // QR], rp[sp.values % QR]
                    rows = a + b if op == "add" else a * b if op == "mul" else \
                        torch.cat([a, b], 1)
                    outs.append(rows if onehot else rows.view(B, BAG_LEN, -1).mean(1))
                o3.zero_grad(set_to_none=True)
                torch.cat(outs, 1).backward(gout)
                o3.step()

            # ---- one checked step of every arm, from equal tables ----
            forward_backward("native")
            forward_backward("torch")
            want = []
            for v in vs["native"]:
                for tab in v.val_list:
                    sl = tab.pending_grads[0]
                    n = int(sl.num_valid.item()) if sl.num_valid is not None else sl.indices.numel()
                    w = tab.weight.cpu().numpy().copy()
                    acc = np.full_like(w, 0.1)
                    ref.apply_adagrad(orc, w, acc, LR, sl.indices[:n].cpu().numpy(),
                                      sl.values[:n].cpu().numpy())
                    want.append(w)
            apply("native")
            apply("torch")
            step_torch()
            dr.status_check()
            got_n = [t.weight.cpu().numpy() for v in vs["native"] for t in v.val_list]
            got_t = [t.weight.cpu().numpy() for v in vs["torch"] for t in v.val_list]
            got_p = [p.detach().cpu().numpy() for pair in pq for p in pair]
            for k, w in enumerate(want):
                assert np.array_equal(got_n[k].view(np.int32), w.view(np.int32)), (tag, k)
                np.testing.assert_allclose(got_t[k], w, rtol=1e-5, atol=1e-7)
                np.testing.assert_allclose(got_p[k], w, rtol=1e-3, atol=1e-6)
            checks[tag] = {
                "native == oracle (bits)": True,
                "torch arm elements differing from the oracle in bits": int(sum(
                    (a.view(np.int32) != w.view(np.int32)).sum() for a, w in zip(got_t, want))),
                "elements": int(sum(w.size for w in want)),
            }
            del want, got_n, got_t, got_p

            # ---- the whole step ----
            steps = {"native": lambda: step_engine("native"), "torch": lambda: step_engine("torch"),
                     "plain torch": step_torch}
            for name in steps:
                steps[name]()                      # warm-up
            for r in range(args.rounds):
                for name in _order(ARMS, r):
                    res.setdefault("%s: train step, %d features, %s ms" % (tag, T, name),
                                   []).append(_clock(steps[name], args.reps))
            # ---- the optimizer step alone, over the same queued slices ----
            saved = {}
            for arm in vs:
                forward_backward(arm)
                saved[arm] = [(tab, list(tab.pending_grads)) for v in vs[arm] for tab in v.val_list]
                for tab, _ in saved[arm]:
                    tab.pending_grads = []

            def apply_only(arm):
                for tab, sls in saved[arm]:
                    tab.pending_grads = list(sls)
                apply(arm)
            for r in range(args.rounds):
                for name in _order(("native", "torch"), r):
                    res.setdefault("%s: apply_gradients alone, %d tables, %s ms"
                                   % (tag, 2 * T, name), []).append(
                        _clock(lambda: apply_only(name), args.reps))
            del vs, opts, pq, o3, saved
            print("%s done" % tag, flush=True)
        torch.cuda.empty_cache()
    # ---- run length: one table, 65 536 positions, apply_gradients alone ----
    # (a run is walked by one lane group; reps // 4 calls per timing: the
    # one-row case takes tens of ms a call)
    vals = torch.randn((ONEHOT, DIM), generator=g, device=dev) * 0.01
    ar = torch.arange(ONEHOT, device=dev)
    for name, idx in (("uniformly random rows", torch.randint(0, QR, (ONEHOT,), generator=g,
                                                               device=dev)),
                      ("128 runs of 512", ar // 512), ("one row", ar * 0)):
        tabs = {a: dr.DenseTable(torch.randn((QR, DIM), generator=g, device=dev)) for a in ARMS[:2]}
        opts = {a: dr.AdagradOptimizer(LR, initial_accumulator_value=0.1) for a in tabs}

        def one(arm):
            tabs[arm].pending_grads.append(dr.IndexedSlices(vals, idx))
            training._NATIVE_DENSE = arm == "native"
            try:
                opts[arm].apply_gradients([tabs[arm]], global_step=1)
            finally:
                training._NATIVE_DENSE = True
        for arm in tabs:
            one(arm)                               # warm-up
        for r in range(args.rounds):
            for arm in _order(ARMS[:2], r):
                res.setdefault("run length, 1 table x %d positions, %s: %s ms"
                               % (ONEHOT, name, arm), []).append(
                    _clock(lambda: one(arm), max(1, args.reps // 4)))
        print("run length %s done" % name, flush=True)
    results = {k: _summary(v) for k, v in sorted(res.items())}
    out = {"features": T, "dim": DIM, "q rows": QR, "r rows": QR, "rounds": args.rounds,
           "reps": args.reps, "optimizer": "Adagrad", "device": torch.cuda.get_device_name(0),
           "checked before timing": checks, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"results": results, "checks": checks}, indent=1, sort_keys=True))
    dr.status_check()


if __name__ == "__main__":
    main()
