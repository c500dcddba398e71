"""Times CAN's co-action unit alone: the forward and the
backward entries against their byte and matrix-core floors, and forward +
backward through autograd, native against DR_CO_ACTION=torch.  Each arm runs in
a child process of its own (the switch is read when the package loads), the
arms alternating over --runs rounds; every child event-times --calls calls
after a warm-up and reports its mean.  Prints one JSON line: per arm and figure
the mean over the runs and their spread, and the floors.

  python tools/co_action_bench.py [--batch 4096] [--positions 100] [--widths 16,8,4]
                                  [--orders 3] [--bias] [--order-indep] [--calls 20] [--runs 3]

The defaults are the reference configuration at a training batch; the mask is
a valid prefix of length U[1, positions], as DIN's batches have it."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))
MFMA_TFLOPS = 158.0                                         # fp32 matrix rate, DESIGN section 29
HBM_TBS = 8.0                                               # peak HBM3E bandwidth of the part


def child(args):
    import torch

    import deeprec_amd as dr
    from deeprec_amd import ops
    dr.load()
    dev = torch.device("cuda", 0)
    B, T, widths, orders = args.batch, args.positions, args.widths, args.orders
    P = ops.co_action_param_len(widths, orders, args.bias, args.order_indep)
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    his = (r(B, T, widths[0]) * 0.5).requires_grad_()
    param = (r(B, P) * widths[0] ** -0.5).requires_grad_()
    lens = torch.randint(1, T + 1, (B,), generator=g, device=dev)
    mask = (torch.arange(T, device=dev)[None, :] < lens[:, None]).float()
    go = r(B, orders * sum(widths[1:]))
    cfg = (widths, orders, args.bias, args.order_indep)
    if not ops.co_action_native_ok(param, his, mask, widths, orders):
        raise SystemExit("co_action_bench: the shape is outside the kernels' set")

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
        his.grad = param.grad = None
        ops.co_action(param, his, mask, *cfg).backward(go)

    out = {"op_ms": timed(op), "live": float(mask.mean())}
    if ops._CO_ACTION_NATIVE:
        dp, dh = param.detach(), his.detach()
        out["fwd_ms"] = timed(lambda: ops.co_action_forward(dp, dh, mask, *cfg))
        out["bwd_ms"] = timed(lambda: ops.co_action_backward(dp, dh, mask, go, *cfg))
    dr.status_check(dev)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--positions", type=int, default=100)
    ap.add_argument("--widths", type=lambda s: tuple(int(d) for d in s.split(",")),
                    default=(16, 8, 4))
    ap.add_argument("--orders", type=int, default=3)
    ap.add_argument("--bias", action="store_true")
    ap.add_argument("--order-indep", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arms", default="native,torch")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    B, T, w, orders = args.batch, args.positions, args.widths, args.orders
    runs = {arm: [] for arm in args.arms.split(",")}
    for _ in range(args.runs):
        for arm in runs:                                    # the arms alternate
            env = dict(os.environ, DR_CO_ACTION=arm)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"]
                                 + sys.argv[1:], env=env, check=True, stdout=subprocess.PIPE)
            runs[arm].append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
    per = sum(a * b + (b if args.bias else 0) for a, b in zip(w[:-1], w[1:]))
    P = per * (orders if args.order_indep else 1)
    # bytes: his and param read and out written (every position, the mask apart); the backward
    # reads grad_out too and writes grad_his and grad_param
    fwd_b = 4.0 * B * (T * w[0] + P + orders * sum(w[1:]))
    bwd_b = fwd_b + 4.0 * B * (T * w[0] + P)
    # flop: 2 B T orders sum_j d(j-1) d(j) for the forward; the backward forms the same products
    # for the chain back and the weight gradient, and the layers below the last again
    mm = 2.0 * B * T * orders * sum(a * b for a, b in zip(w[:-1], w[1:]))
    res = {"op": "co_action", "batch": B, "positions": T, "widths": list(w), "orders": orders,
           "bias": args.bias, "order_indep": args.order_indep, "calls": args.calls,
           "runs": args.runs,
           "byte_floor_ms": {"fwd_ms": round(fwd_b / (HBM_TBS * 1e9), 4),
                             "bwd_ms": round(bwd_b / (HBM_TBS * 1e9), 4)},
           "mfma_floor_ms": {"fwd_ms": round(mm / (MFMA_TFLOPS * 1e9), 4),
                             "bwd_ms": round(3 * mm / (MFMA_TFLOPS * 1e9), 4)}}
    for arm, rs in runs.items():
        for key in rs[0]:
            v = [r[key] for r in rs]
            res["%s_%s" % (arm, key)] = {"mean": round(sum(v) / len(v), 4), "min": round(min(v), 4),
                                         "max": round(max(v), 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
