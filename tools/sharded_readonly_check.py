"""Multi-process check of the native sharded engines' read-only forward
(dr_sharded_forward with DR_SHARDED_READ_ONLY), every kind.

  python tools/sharded_readonly_check.py [--world 2]

The parent never touches the GPU; it spawns `world` processes that all use
cuda:0 and a gloo process group (Comm.host_staged: the gloo collectives
behind the dr_comm callbacks).  Rank r holds the EV shards of the keys
k % world == r out of 0 .. N_KEYS-1; ids are drawn from [0, ID_SPACE), so
about a third are absent everywhere.  Checks, bit for bit:
  * kinds rccl, fixed and xgmi, one-hot; rccl and fixed also multi-hot mean
    bags and bf16 EVs (fp32 and bf16 outputs): the read-only forward == this
    rank's batch looked up inside read_only_lookups() in a full local copy
    of every table (embedding_lookup_sparse_multi), and every shard's
    total_count and export are what they were;
  * DR_SHARDED_READ_ONLY with need_grad returns DR_INVALID_ARGUMENT, on every
    rank, before any exchange;
  * a backward after a read-only forward refuses.
The parent prints one JSON line per rank; exit code != 0 on any mismatch.
The first rank that fails or stalls ends the others.
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, D, B, N_KEYS, ID_SPACE, DEFAULT = 3, 16, 37, 100, 150, 0.125


def _vals(t, keys):
    k = np.asarray(keys, np.float64)[:, None]
    return np.cos(0.013 * k + 0.7 * t + 0.05 * np.arange(D)[None, :]).astype(np.float32)


def _onehot_ids(seed, rank):
    ids = np.random.default_rng(31 + 1000 * seed + rank).integers(0, ID_SPACE, (T, B))
    ids[:, :4] = 17 + seed          # a repeated id in every table
    return ids.astype(np.int64)


def _bags(seed, rank):
    rng = np.random.default_rng(77 + 1000 * seed + rank)
    lens = rng.integers(0, 4, (T, B))
    lens[:, 0] = 3
    lens[:, 3] = 0
    ids, offs = [], []
    for t in range(T):
        o = np.concatenate([[0], np.cumsum(lens[t])]).astype(np.int32)
        v = rng.integers(0, ID_SPACE, int(o[-1])).astype(np.int64)
        v[:3] = 3                                # a hot key
        ids.append(v)
        offs.append(o)
    return ids, offs, lens


def worker(rank, world, port, q):
    import ctypes as C

    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import deeprec_amd as dr
    from deeprec_amd import _lib
    from deeprec_amd._lib import COMBINERS, lib, ptr, stream_handle
    from deeprec_amd.embedding_ops import SparseTensor, embedding_lookup_sparse_multi
    from deeprec_amd.sharded import Comm, NativeShardedLookup
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dr.load()
    dr.set_validate(True)
    allk = np.arange(N_KEYS, dtype=np.int64)
    res = {"rank": rank, "world": world, "checks": []}
    ok = True

    def check(name, same):
        nonlocal ok
        same = bool(same)
        res["checks"].append([name, same])
        ok = ok and same

    def same_bits(a, b):
        a, b = a.detach().contiguous(), b.detach().contiguous()
        return a.dtype == b.dtype and a.shape == b.shape and \
            np.array_equal(a.view(torch.uint8).cpu().numpy(), b.view(torch.uint8).cpu().numpy())

    def evset(tag, value_dtype=torch.float32, full=False):
        evs = []
        for t in range(T):
            ev = dr.EmbeddingVariable("%s%d_%d" % (tag, rank, t), D, DEFAULT, capacity=64,
                                      device=dev, value_dtype=value_dtype)
            k = allk if full else allk[allk % world == rank]
            ev.insert(torch.as_tensor(k, device=dev),
                      torch.as_tensor(_vals(t, k), device=dev).to(value_dtype))
            evs.append(ev)
        return evs

    def state(evs):
        out = []
        for ev in evs:
            k, v, ver, fr = ev.export()
            out.append((int(ev.total_count()[0]), k.cpu().numpy(),
                        v.contiguous().view(torch.uint8).cpu().numpy(), fr.cpu().numpy()))
        return out

    def same_state(a, b):
        return all(x[0] == y[0] and all(np.array_equal(p, r) for p, r in zip(x[1:], y[1:]))
                   for x, y in zip(a, b))

    def ref_onehot(full, it, out_dtype=None):
        ind1 = torch.stack([torch.arange(B, device=dev),
                            torch.zeros(B, dtype=torch.int64, device=dev)], 1)
        sps = [SparseTensor(ind1, it[t], (B, 1)) for t in range(T)]
        with torch.no_grad(), dr.read_only_lookups():
            if out_dtype is None:
                return embedding_lookup_sparse_multi(full, sps, combiner="sum")
            return embedding_lookup_sparse_multi(full, sps, combiner="sum", out_dtype=out_dtype)

    comm = Comm.host_staged()
    sets = {torch.float32: (evset("sh"), evset("fu", full=True)),
            torch.bfloat16: (evset("bs", torch.bfloat16), evset("bf", torch.bfloat16, full=True))}
    g = torch.ones((B, T * D), dtype=torch.float32, device=dev)
    for kind in ("rccl", "fixed", "xgmi"):
        shard, full = sets[torch.float32]
        s0 = state(shard)
        eng = NativeShardedLookup(comm, shard, dev, kind=kind, batch=B, max_ids=4 * B)
        it = torch.as_tensor(_onehot_ids(0, rank), device=dev)
        out = eng.forward(it, combiner="sum", read_only=True)
        torch.cuda.synchronize()
        check("%s_onehot" % kind, same_bits(out, ref_onehot(full, it)))
        # a backward after it refuses (no exchange is started: no rank waits)
        try:
            eng.backward(g)
            check("%s_backward_refuses" % kind, False)
        except _lib.DeepRecError as e:
            check("%s_backward_refuses" % kind, e.code == _lib.INVALID_ARGUMENT)
        # the flag with need_grad: refused by the C entry on every rank
        ka = (C.c_int64 * (T + 1))(*[t * B for t in range(T + 1)])
        o2 = torch.empty((B, T * D), dtype=torch.float32, device=dev)
        rc = lib().dr_sharded_forward(eng.h, ptr(it.reshape(-1)), ka, None, B, COMBINERS["sum"],
                                      1, _lib.SHARDED_READ_ONLY, ptr(o2), stream_handle(dev))
        check("%s_need_grad_refused" % kind, rc == _lib.INVALID_ARGUMENT)
        try:
            eng.forward(it, need_grad=True, read_only=True)
            check("%s_need_grad_value_error" % kind, False)
        except ValueError:
            check("%s_need_grad_value_error" % kind, True)
        # the context alone selects the read-only forward
        it = torch.as_tensor(_onehot_ids(1, rank), device=dev)
        with dr.read_only_lookups():
            out = eng.forward(it, combiner="sum")
        torch.cuda.synchronize()
        check("%s_onehot_context" % kind, same_bits(out, ref_onehot(full, it)))
        if kind != "xgmi":
            ids, offs, lens = _bags(0, rank)
            its = [torch.as_tensor(x, device=dev) for x in ids]
            ot = [torch.as_tensor(o, device=dev) for o in offs]
            sps = []
            for t in range(T):
                rows = np.repeat(np.arange(B), lens[t])
                ind = np.stack([rows, np.zeros_like(rows)], 1).astype(np.int64)
                sps.append(SparseTensor(torch.as_tensor(ind, device=dev), its[t], (B, 4)))
            with torch.no_grad(), dr.read_only_lookups():
                ref = embedding_lookup_sparse_multi(full, sps, combiner="mean")
            out = eng.forward(its, bag_offs=ot, combiner="mean", read_only=True)
            torch.cuda.synchronize()
            check("%s_bags_mean" % kind, same_bits(out, ref))
        check("%s_shards_unchanged" % kind, same_state(s0, state(shard)))
        eng.close()
        if kind != "xgmi":
            sb, fb = sets[torch.bfloat16]
            b0 = state(sb)
            eb = NativeShardedLookup(comm, sb, dev, kind=kind, batch=B, max_ids=B)
            it = torch.as_tensor(_onehot_ids(2, rank), device=dev)
            o32 = eb.forward(it, combiner="sum", read_only=True)
            check("%s_bf16_fp32" % kind, same_bits(o32, ref_onehot(fb, it)))
            o16 = eb.forward(it, combiner="sum", out_dtype=torch.bfloat16, read_only=True)
            check("%s_bf16_bf16" % kind, same_bits(o16, ref_onehot(fb, it, torch.bfloat16)))
            check("%s_bf16_shards_unchanged" % kind, same_state(b0, state(sb)))
            eb.close()
    dr.status_check()
    comm.close()
    res["ok"] = ok
    q.put(json.dumps(res))   # the parent prints: one whole line per rank
    dist.barrier()
    dist.destroy_process_group()
    if not ok:
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--timeout", type=float, default=100.0)
    args = ap.parse_args()
    import multiprocessing as mp
    import queue
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, args.world, port, q)) for r in range(args.world)]
    for p in procs:
        p.start()
    # one line per rank; a rank that dies (or the deadline) ends the others,
    # which would otherwise wait for it in a collective
    deadline = time.monotonic() + args.timeout
    got = 0
    while got < len(procs) and time.monotonic() < deadline:
        try:
            print(q.get(timeout=0.5), flush=True)
            got += 1
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    if got == len(procs):
        for p in procs:
            p.join(30)
    for p in procs:
        if p.is_alive():
            p.terminate()
    for p in procs:
        p.join(10)
    codes = [p.exitcode for p in procs]
    sys.exit(0 if got == len(procs) and all(c == 0 for c in codes) else 1)


if __name__ == "__main__":
    main()
