"""Times the multi-head self-attention op alone at the BST
shape: forward + backward through autograd over the column blocks of a packed
projection, event-timed per call, the native kernels and the torch composition
alternating in one process.  Prints one JSON line.

  python tools/mha_bench.py [--batch 4096] [--len 101] [--heads 4] [--head-dim 16]
                            [--calls 20] [--no-torch]

--no-torch runs the native arm only (for a profiler's kernel trace)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--len", type=int, default=101)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--head-dim", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    import deeprec_amd as dr
    from deeprec_amd import ops
    dr.load()
    dev = torch.device("cuda", 0)
    B, T, heads, E = args.batch, args.len, args.heads, args.heads * args.head_dim
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    packed = torch.relu(torch.randn(B, T, 3 * E, generator=g, device=dev)).requires_grad_()
    go = torch.randn(B, T, E, generator=g, device=dev)
    lens = torch.randint(1, T + 1, (B,), generator=g, device=dev).to(torch.int32)
    arms = {"native": ops._MultiheadAttentionFn.apply}
    if not args.no_torch:
        arms["torch"] = ops._multihead_attention_torch
    if not ops.mha_native_ok(packed[..., :E], heads):
        raise SystemExit("mha_bench: the shape is outside the kernels' set")

    def call(fn):
        packed.grad = None
        out = fn(packed[..., :E], packed[..., E:2 * E], packed[..., 2 * E:], lens, heads)
        out.backward(go)
        return out

    ms = {name: [] for name in arms}
    for i in range(args.warmup + args.calls):
        for name, fn in arms.items():                       # the arms alternate
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(fn)
            b.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[name].append(a.elapsed_time(b))
    dr.status_check(dev)
    res = {"op": "mha fwd+bwd", "batch": B, "len": T, "heads": heads, "head_dim": args.head_dim,
           "calls": args.calls}
    for name, v in ms.items():
        res[name + "_ms"] = {"mean": round(sum(v) / len(v), 4), "min": round(min(v), 4),
                             "max": round(max(v), 4)}
    if "torch" in ms:
        err = (call(arms["native"]) - call(arms["torch"])).abs().max()
        res["max_abs_diff"] = float(err)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
