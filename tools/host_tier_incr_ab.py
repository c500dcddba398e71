"""Measurement of incremental checkpoints on a tiered key space (DESIGN
section 17), with tools/host_tier_ab.py's method.  Every row is set against a
yardstick measured in the same run:

  demote   demote_to of 10 % of the keys, tracking on (every key marked, so
           every victim carries bit 16) | the same call on an EV that is not
           tracking: the difference is the bitmap read in the victims' export
  export   export_updated with 65 536 flagged keys in a tier of 10 % of the
           table | export_updated of the same keys, resident, on the untiered
           twin: the host store's masked read and the copy to the device
           against the device scan
  promote  promote of those 65 536 keys, tracking on and every flag set | the
           same call, tracking off: the difference is the mark in the one launch
  step     one training step (one-hot lookup of 65 536 resident keys, backward,
           SGD apply_gradients) on the tiered EV with a non-empty tier and no
           tier hit, tracking by row | the same step with tracking off, and on
           the untiered twin tracking by row
  save     save_incremental of 65 536 marked keys, half of them in the tier |
           the twin's save_incremental of the same keys

One table (4 M x 128 fp32 by default) with an Adagrad slot column, versions
drawn from 1 000 distinct steps.  The cases alternate inside each of five
rounds (fresh tables per round); medians and max - min are reported.  Each
result is checked: the flags the store holds, the promoted keys' marks, the
exports field by field, the two deltas byte for byte.  Host clock around calls
that end in a device synchronise.

usage: python tools/host_tier_incr_ab.py [--rows 4000000] [--dim 128] [--rounds 5]
           [--out profiles/host_tier_incr.json]"""
import argparse
import ctypes as C
import filecmp
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))

import torch  # noqa: E402

from host_tier_ab import BATCH, STEPS, _clock, _summary  # noqa: E402

UPDATED = 1 << 16


def _table(dr, dev, name, R, D, versions, tiered):
    evict = dr.KeyBudgetEvict(R, "lru", steps_to_live=10**9) if tiered \
        else dr.GlobalStepEvict(10**9)
    so = dr.StorageOption(dr.StorageType.HBM_DRAM, incremental=True) if tiered else None
    ev = dr.EmbeddingVariable(name, D, 0.0, device=dev, capacity=R,
                              ev_option=dr.EmbeddingVariableOption(evict_option=evict,
                                                                   storage_option=so))
    slot = ev.slot("Adagrad", 0.1)
    ev.insert_synthetic(0, R, seed=77)
    slot.insert_synthetic(0, R, seed=78)
    keys = torch.arange(0, R, dtype=torch.int64, device=dev)
    step = 1 << 18
    zeros = torch.zeros((step, D), device=dev)
    for i in range(0, R, step):                 # existing rows are kept: only the version lands
        part = keys[i:i + step]
        ev.insert(part, zeros[:part.numel()], versions[i:i + step])
    return ev, slot


def _flagged(dr, ev):
    n = C.c_int64(0)
    with ev._lock:
        dr._lib.check(dr._lib.lib().dr_host_tier_count_masked(ev._tier, UPDATED, C.byref(n)))
    return n.value


def _step(dr, opt, ev, ind, batch, grad, gs):
    out = dr.embedding_lookup_sparse(ev, dr.SparseTensor(ind, batch, (BATCH, 1)), combiner="sum")
    out.backward(grad)
    opt.apply_gradients([ev], global_step=gs)
    return out.detach()


def one_round(args, dr, ck, dev, r, res):
    R, D = args.rows, args.dim
    g = torch.Generator(device=dev)
    g.manual_seed(31 + r)
    versions = torch.randint(1, STEPS + 1, (R,), generator=g, device=dev, dtype=torch.int64)
    on, on_slot = _table(dr, dev, "incr_ab_on_%d" % r, R, D, versions, True)
    off, off_slot = _table(dr, dev, "incr_ab_off_%d" % r, R, D, versions, True)
    twin, twin_slot = _table(dr, dev, "incr_ab_twin_%d" % r, R, D, versions, False)
    allkeys = torch.arange(0, R, dtype=torch.int64, device=dev)
    for ev in (on, twin):
        ev.track_updates(by_row=True)
        ev.track_removals()
    on.mark_updated(allkeys)
    E = R // 10
    order = ("on", "off") if r % 2 == 0 else ("off", "on")

    def add(name, t):
        res.setdefault(name, []).append(t)

    # demote 10 %: tracking on, every victim marked | tracking off
    for what in order:
        ev = on if what == "on" else off
        t, n = _clock(lambda: ev.demote_to(R - E, compact=False))
        assert n == E and ev.tier_count() == E, (what, n, E)
        add("demote_to 10%% tracking %s ms" % what, t)
    assert _flagged(dr, on) == E and _flagged(dr, off) == 0
    with on._lock:
        victims = torch.from_numpy(on._tier_export(columns=())[0]).to(dev)
    with off._lock:
        assert torch.equal(victims, torch.from_numpy(off._tier_export(columns=())[0]).to(dev))
    # export_updated: 65 536 flagged keys in the tier | the same keys resident in the twin
    fk = victims[torch.randperm(E, generator=g, device=dev)[:BATCH]].contiguous()
    on.clear_updated()
    assert _flagged(dr, on) == 0 and on.updated_count() == 0
    on.mark_updated(fk)                         # the public route: flags in the store
    twin.mark_updated(fk)
    assert _flagged(dr, on) == BATCH and on._export_updated_hbm()[0].numel() == 0
    for what in order:
        ev = on if what == "on" else twin
        t, out = _clock(ev.export_updated)
        add("export_updated 65536 %s ms" % ("in the tier" if ev is on else "resident (twin)"), t)
        if ev is on:
            got = out
    for x, y in zip(got, twin.export_updated()):
        assert torch.equal(x, y), "export_updated differs from the twin's"
    # promote the flagged keys: tracking on, every flag set | tracking off
    for what in order:
        ev = on if what == "on" else off
        t, n = _clock(lambda: ev.promote(fk))
        assert n == BATCH and ev.tier_count() == E - BATCH
        add("promote 65536 tracking %s ms" % what, t)
    assert _flagged(dr, on) == 0
    assert torch.equal(on._export_updated_hbm()[0], torch.sort(fk)[0]), \
        "the promoted keys are not the marked keys"
    # one training step, resident keys, non-empty tier, no tier hit
    hbm = torch.ones(R, dtype=torch.bool, device=dev)
    hbm[victims] = False
    hbm[fk] = True
    pool = allkeys[hbm]
    batch = pool[torch.randperm(pool.numel(), generator=g, device=dev)[:BATCH]].contiguous()
    del hbm, pool
    ind = torch.stack([torch.arange(BATCH, device=dev),
                       torch.zeros(BATCH, dtype=torch.int64, device=dev)], 1)
    grad = torch.randint(-2, 3, (BATCH, D), generator=g, device=dev).to(torch.float32)
    opt = dr.GradientDescentOptimizer(0.5)
    tiers = (on.tier_count(), off.tier_count())
    outs = [_step(dr, opt, ev, ind, batch, grad, STEPS + 1) for ev in (on, off, twin)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert (on.tier_count(), off.tier_count()) == tiers     # no tier hit
    assert torch.isin(torch.unique(batch), on._export_updated_hbm()[0]).all()

    def steps(ev):      # (the same global steps on every table: the deltas below stay equal)
        gs = [STEPS + 1]

        def run():
            gs[0] += 1
            _step(dr, opt, ev, ind, batch, grad, gs[0])
        return run
    for what in order + ("twin",):
        ev = {"on": on, "off": off, "twin": twin}[what]
        t, _ = _clock(steps(ev), reps=10)
        add("step %s ms" % {"on": "tiered, tracking by row", "off": "tiered, tracking off",
                            "twin": "untiered twin, tracking by row"}[what], t)
    # save_incremental: 65 536 marked keys, half in the tier | the twin
    for ev in (on, twin):
        ev.clear_updated()
    with on._lock:
        tk = torch.from_numpy(on._tier_export(columns=())[0]).to(dev)
    mk = torch.cat([tk[torch.randperm(tk.numel(), generator=g, device=dev)[:BATCH // 2]],
                    fk[:BATCH // 2]]).contiguous()
    for ev in (on, twin):
        ev.mark_updated(mk)
    assert _flagged(dr, on) == BATCH // 2
    tmp = tempfile.mkdtemp(prefix="incr_ab_")
    try:
        paths = {}
        for what in order:
            ev, slot = (on, on_slot) if what == "on" else (twin, twin_slot)
            name = "tiered" if ev is on else "twin"
            t, p = _clock(lambda: ck.save_incremental(os.path.join(tmp, name),
                                                      {"emb": ev, "emb/Adagrad": slot}))
            paths[name] = p
            add("save_incremental 65536 %s ms" % name, t)
        for ext in (".index", ".data-00000-of-00001"):
            assert filecmp.cmp(paths["tiered"] + ext, paths["twin"] + ext, shallow=False), ext
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    del on, on_slot, off, off_slot, twin, twin_slot
    dr.flush_releases()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4000000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_tier_incr.json"))
    args = ap.parse_args()
    if args.rows // 10 < 2 * BATCH:
        ap.error("--rows: 10 %% of the table must hold two batches of %d keys" % BATCH)
    import deeprec_amd as dr
    from deeprec_amd import checkpoint as ck
    dev = torch.device("cuda", 0)
    res = {}
    for r in range(args.rounds):
        one_round(args, dr, ck, dev, r, res)
        print("round %d done" % r, flush=True)
    out = {"rows": args.rows, "dim": args.dim, "rounds": args.rounds, "batch": BATCH,
           "device": torch.cuda.get_device_name(0),
           "results": {k: _summary(v) for k, v in sorted(res.items())}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["results"], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
