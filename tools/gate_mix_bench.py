"""Times the gate softmax / expert mixing op alone: the two
kernels, and forward + backward through autograd over strided views, native
against DR_GATE_MIX=torch.  Each arm runs in a child process of its own (the
switch is read when the package loads), the arms alternating over --runs
rounds; every child event-times --calls calls after a warm-up and reports its
mean.  Prints one JSON line: per arm and figure the mean over the runs and
their spread, and the kernels' byte floors.

  python tools/gate_mix_bench.py [--batch 65536] [--tasks 2] [--experts 8] [--width 128]
                                 [--ple] [--calls 50] [--runs 3]

--ple gives every task but the last a two-expert view (its own and the last
expert) and the last task every expert, as a PLE level below the last does."""
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
    B, K, E, H = args.batch, args.tasks, args.experts, args.width
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    # the op's inputs in a model: column blocks of wider Linear outputs
    zw = torch.randn(B, K * E + 8, generator=g, device=dev).requires_grad_()
    hw = torch.randn(B, E * H + 8, generator=g, device=dev).requires_grad_()
    go = torch.randn(B, K, H, generator=g, device=dev)
    select = None
    if args.ple:
        select = torch.zeros(K, E, dtype=torch.bool)
        for k in range(K - 1):
            select[k, k % E] = select[k, E - 1] = True
        select[K - 1] = True
    z, h = zw[:, :K * E].view(B, K, E), hw[:, :E * H].view(B, E, H)
    if not ops.gate_mix_native_ok(z, h):
        raise SystemExit("gate_mix_bench: the shape is outside the kernels' set")

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
        zw.grad = hw.grad = None
        ops.gate_mix(z, h, select).backward(go)

    res = {"op_ms": timed(op)}
    if ops._GATE_MIX_NATIVE:
        zd, hd = z.detach(), h.detach()
        _, gates = ops.gate_mix_forward(zd, hd, select)
        res["fwd_ms"] = timed(lambda: ops.gate_mix_forward(zd, hd, select))
        res["bwd_ms"] = timed(lambda: ops.gate_mix_backward(hd, gates, go, select))
    dr.status_check(dev)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--tasks", type=int, default=2)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--ple", action="store_true")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    B, K, E, H = args.batch, args.tasks, args.experts, args.width
    runs = {"native": [], "torch": []}
    for _ in range(args.runs):
        for arm in runs:                                    # the arms alternate
            env = dict(os.environ, DR_GATE_MIX=arm)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"]
                                 + sys.argv[1:], env=env, check=True, stdout=subprocess.PIPE)
            runs[arm].append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
    floor = {"fwd_ms": 4 * B * ((E + K) * H + 2 * K * E) / (COPY_TBS * 1e9),
             "bwd_ms": 4 * B * ((2 * E + K) * H + 2 * K * E) / (COPY_TBS * 1e9)}
    res = {"op": "gate_mix", "batch": B, "tasks": K, "experts": E, "width": H, "ple": args.ple,
           "calls": args.calls, "runs": args.runs,
           "byte_floor_ms": {k: round(v, 4) for k, v in floor.items()}}
    for arm, rs in runs.items():
        for key in rs[0]:
            v = [r[key] for r in rs]
            res["%s_%s" % (arm, key)] = {"mean": round(sum(v) / len(v), 4), "min": round(min(v), 4),
                                         "max": round(max(v), 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
