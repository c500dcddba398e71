"""Times the bilinear interaction alone: the forward and the
backward entries against their HBM floors, and forward + backward through
autograd, native against DR_BILINEAR=torch.  Each arm runs in a child process
of its own (the switch is read when the package loads), the arms alternating
over --runs rounds; every child event-times --calls calls after a warm-up and
reports its mean.  Prints one JSON line: per arm and figure the mean over the
runs and their spread, the floors, and the native entries' ratio to them.

  python tools/bilinear_bench.py [--batch 4096] [--fields 26] [--width 16]
                                 [--kind interaction] [--no-scale] [--calls 20] [--runs 3]

The floor of a launch is the bytes it must move at the 8 TB/s HBM peak: the
forward reads x, scale and W and writes out; the backward reads grad_out, x,
scale and W once and writes grad_x, grad_scale and grad_W."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))
HBM_PEAK_GBS = 8000.0


def child(args):
    import torch

    import deeprec_amd as dr
    from deeprec_amd import ops
    dr.load()
    dev = torch.device("cuda", 0)
    B, m, D, kind = args.batch, args.fields, args.width, args.kind
    P = m * (m - 1) // 2
    g = torch.Generator(device=dev)
    g.manual_seed(2019)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    x = r(B, m, D).requires_grad_()
    w = (r({"all": 1, "each": m, "interaction": P}[kind], D, D) * D ** -0.5).requires_grad_()
    scale = None if args.no_scale else torch.rand(B, m, generator=g, device=dev).requires_grad_()
    go = r(B, P, D)
    if not ops.bilinear_native_ok(x, w, scale):
        raise SystemExit("bilinear_bench: the shape is outside the kernels' set")

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
        for t in (x, w, scale):
            if t is not None:
                t.grad = None
        ops.bilinear_interaction(x, w, kind, scale).backward(go)

    out = {"op_ms": timed(op)}
    if ops._BILINEAR_NATIVE:
        dx, dw = x.detach(), w.detach()
        ds = None if scale is None else scale.detach()
        out["fwd_ms"] = timed(lambda: ops.bilinear_forward(dx, dw, kind, ds))
        out["bwd_ms"] = timed(lambda: ops.bilinear_backward(dx, dw, kind, go, ds))
    dr.status_check(dev)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--kind", default="interaction", choices=["all", "each", "interaction"])
    ap.add_argument("--no-scale", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arms", default="native,torch")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    B, m, D = args.batch, args.fields, args.width
    P = m * (m - 1) // 2
    runs = {arm: [] for arm in args.arms.split(",")}
    for _ in range(args.runs):
        for arm in runs:                                    # the arms alternate
            env = dict(os.environ, DR_BILINEAR=arm)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"]
                                 + sys.argv[1:], env=env, check=True, stdout=subprocess.PIPE)
            runs[arm].append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
    n_w = {"all": 1, "each": m, "interaction": P}[args.kind] * D * D
    small = B * m * D + (0 if args.no_scale else B * m) + n_w    # x, scale, W: floats
    floor = lambda floats: 4.0 * floats / (HBM_PEAK_GBS * 1e6)   # noqa: E731  (ms)
    floors = {"fwd_ms": floor(B * P * D + small), "bwd_ms": floor(B * P * D + 2 * small)}
    res = {"op": "bilinear_interaction", "kind": args.kind, "batch": B, "fields": m, "width": D,
           "scale": not args.no_scale, "calls": args.calls, "runs": args.runs,
           "hbm_floor_ms": {k: round(v, 4) for k, v in floors.items()}}
    for arm, rs in runs.items():
        for key in rs[0]:
            v = [r[key] for r in rs]
            res["%s_%s" % (arm, key)] = {"mean": round(sum(v) / len(v), 4), "min": round(min(v), 4),
                                         "max": round(max(v), 4)}
    for key, fl in floors.items():
        if "native_" + key in res:
            res["native_%s_over_floor" % key[:3]] = round(res["native_" + key]["mean"] / fl, 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
