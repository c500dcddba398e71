"""Times the layer-norm / relu / mask-multiply op alone: the
two directions of the kernels against their byte floors, and forward +
backward through autograd, native against DR_LAYER_NORM=torch.  Each arm runs
in a child process of its own (the switch is read when the package loads), the
arms alternating over --runs rounds; every child event-times --calls calls
after a warm-up and reports its mean.  Prints one JSON line: per arm and
figure the mean over the runs and their spread, and the byte floors.

  python tools/layer_norm_bench.py [--batch 65536] [--width 416] [--masks 3] [--relu]
                                   [--residual] [--calls 50] [--runs 3]

--masks 0 is the op without a mask (out [B, D]).  The defaults are MaskNet's
parallel embedding block; --width 512 --masks 1 --relu is a serial block."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))
COPY_TBS = 6.33                                             # the copy ceiling, DESIGN section 5


def child(args):
    import torch

    import deeprec_amd as dr
    from deeprec_amd import ops
    dr.load()
    dev = torch.device("cuda", 0)
    B, D, P = args.batch, args.width, args.masks
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    x, res = r(B, D).requires_grad_(), r(B, D).requires_grad_() if args.residual else None
    mask = r(B, P, D).requires_grad_() if P else None
    gain, bias = (1 + 0.5 * r(D)).requires_grad_(), r(D).requires_grad_()
    go = r(B, P, D) if P else r(B, D)
    if not ops.layer_norm_native_ok(x, gain, bias, res, mask):
        raise SystemExit("layer_norm_bench: the shape is outside the kernels' set")

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

    leaves = [t for t in (x, res, mask, gain, bias) if t is not None]

    def op():
        for t in leaves:
            t.grad = None
        ops.layer_norm(x, gain, bias, 1e-8, res, mask, args.relu).backward(go)

    out = {"op_ms": timed(op)}
    if ops._LAYER_NORM_NATIVE:
        d = [None if t is None else t.detach() for t in (x, gain, bias, res, mask)]
        _, saved = ops.layer_norm_forward(d[0], d[1], d[2], 1e-8, d[3], d[4], args.relu)
        out["fwd_ms"] = timed(lambda: ops.layer_norm_forward(d[0], d[1], d[2], 1e-8, d[3], d[4],
                                                             args.relu))
        out["bwd_ms"] = timed(lambda: ops.layer_norm_backward(d[0], d[1], d[2], saved, go, d[3],
                                                              d[4], args.relu))
    dr.status_check(dev)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--masks", type=int, default=3)
    ap.add_argument("--relu", action="store_true")
    ap.add_argument("--residual", action="store_true")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    B, D, P, R = args.batch, args.width, args.masks, int(args.residual)
    runs = {"native": [], "torch": []}
    for _ in range(args.runs):
        for arm in runs:                                    # the arms alternate
            env = dict(os.environ, DR_LAYER_NORM=arm)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"]
                                 + sys.argv[1:], env=env, check=True, stdout=subprocess.PIPE)
            runs[arm].append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
    # rows of D floats each direction moves: forward reads x (residual, P masks) and writes
    # max(P, 1) outputs; backward reads x (residual, P masks) and max(P, 1) gradients and
    # writes dx and P mask gradients; (mean, rstd) per row both ways
    floor = {"fwd_ms": 4 * B * ((1 + R + 2 * P + (P == 0)) * D + 2) / (COPY_TBS * 1e9),
             "bwd_ms": 4 * B * ((2 + R + 3 * P + (P == 0)) * D + 2) / (COPY_TBS * 1e9)}
    res = {"op": "layer_norm", "batch": B, "width": D, "masks": P, "relu": args.relu,
           "residual": args.residual, "calls": args.calls, "runs": args.runs,
           "byte_floor_ms": {k: round(v, 4) for k, v in floor.items()}}
    for arm, rs in runs.items():
        for key in rs[0]:
            v = [r[key] for r in rs]
            res["%s_%s" % (arm, key)] = {"mean": round(sum(v) / len(v), 4), "min": round(min(v), 4),
                                         "max": round(max(v), 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
