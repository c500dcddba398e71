"""Times one CIN layer alone: the forward and the backward
entries against their matrix-core floors, and forward + backward through
autograd, native against DR_CIN=torch.  Each arm runs in a child process of
its own (the switch is read when the package loads), the arms alternating over
--runs rounds; every child event-times --calls calls after a warm-up and
reports its mean.  Prints one JSON line: per arm and figure the mean over the
runs and their spread, and the floors.

  python tools/cin_bench.py [--batch 4096] [--fields 26] [--maps-in 128] [--maps-out 128]
                            [--width 16] [--calls 20] [--runs 3]

The defaults are a hidden layer of xDeepFM at sizes (128, 128); --maps-in 26
is its first layer (xk is x0).  At --batch 65536 the torch arm's outer product
is chunked (ops.CIN_TORCH_Z_BYTES)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))
MFMA_TFLOPS = 158.0                                         # fp32 matrix rate, DESIGN section 29


def child(args):
    import torch

    import deeprec_amd as dr
    from deeprec_amd import ops
    dr.load()
    dev = torch.device("cuda", 0)
    B, m, Hk, Hn, D = args.batch, args.fields, args.maps_in, args.maps_out, args.width
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    x0 = r(B, m, D).requires_grad_()
    xk = x0 if Hk == m else r(B, Hk, D).requires_grad_()
    w, bias = (r(Hn, Hk, m) * (Hk * m) ** -0.5).requires_grad_(), r(Hn).requires_grad_()
    go = r(B, Hn, D)
    if not ops.cin_native_ok(x0, xk, w):
        raise SystemExit("cin_bench: the shape is outside the kernels' set")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.calls

    def op():
        for t in (x0, xk, w, bias):
            t.grad = None
        ops.cin_layer(x0, xk, w, bias).backward(go)

    out = {"op_ms": timed(op)}
    if ops._CIN_NATIVE:
        d0, dw, db = x0.detach(), w.detach(), bias.detach()
        dk = d0 if xk is x0 else xk.detach()
        out["fwd_ms"] = timed(lambda: ops.cin_forward(d0, dk, dw, db))
        out["bwd_ms"] = timed(lambda: ops.cin_backward(d0, dk, dw, go))
    dr.status_check(dev)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--maps-in", type=int, default=128)
    ap.add_argument("--maps-out", type=int, default=128)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arms", default="native,torch")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    B, m, Hk, Hn, D = args.batch, args.fields, args.maps_in, args.maps_out, args.width
    runs = {arm: [] for arm in args.arms.split(",")}
    for _ in range(args.runs):
        for arm in runs:                                    # the arms alternate
            env = dict(os.environ, DR_CIN=arm)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"]
                                 + sys.argv[1:], env=env, check=True, stdout=subprocess.PIPE)
            runs[arm].append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
    # 2 B D Hn Hk m4 flop (m4 = m rounded up to 4) each for the forward, the input gradients
    # and the weight gradient, at the fp32 matrix rate
    gemm = 2.0 * B * D * Hn * Hk * (4 * ((m + 3) // 4)) / (MFMA_TFLOPS * 1e9)
    res = {"op": "cin_layer", "batch": B, "fields": m, "maps_in": Hk, "maps_out": Hn, "width": D,
           "calls": args.calls, "runs": args.runs,
           "mfma_floor_ms": {"fwd_ms": round(gemm, 4), "bwd_ms": round(2 * gemm, 4)}}
    for arm, rs in runs.items():
        for key in rs[0]:
            v = [r[key] for r in rs]
            res["%s_%s" % (arm, key)] = {"mean": round(sum(v) / len(v), 4), "min": round(min(v), 4),
                                         "max": round(max(v), 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
