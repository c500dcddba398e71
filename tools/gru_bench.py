"""Times DIEN's two recurrent cells at its shape on one MI355X (DESIGN section
25): the four launches of the native arm (GRU and AUGRU, forward and
backward: dr_gru_seq_forward / _backward, csrc/gru.hip) by device events, and
the torch composition of the same contract (ops._gru_sequence_torch, the
DR_GRU=torch arm) forward + backward, on the same inputs; checks that the two
arms agree.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats --
python tools/gru_bench.py --no-torch` the kernel times come from the trace.

  python tools/gru_bench.py [--batch 4096] [--maxlen 100] [--dim 18] [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deeprec-1_amd"))


def timed(fn, iters, warmup=3):
    """Mean device time of fn in ms (events around `iters` back-to-back calls)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--maxlen", type=int, default=100)
    ap.add_argument("--dim", type=int, default=18, help="embedding dim D; the cells' H = 2 D")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch arm")
    args = ap.parse_args()
    import deeprec_amd as dr
    from deeprec_amd import ops
    dr.load()
    if not torch.cuda.is_available():
        raise SystemExit("gru_bench needs the MI355X")
    dev = torch.device("cuda", 0)
    B, T, H = args.batch, args.maxlen, 2 * args.dim
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    lens = torch.randint(1, T + 1, (B,), generator=g, device=dev).to(torch.int32)
    xp = rn(B, T, 3 * H)
    xp[:, :, :2 * H] += 1.0                                    # gates bias 1
    lim = (6.0 / (3 * H)) ** 0.5
    wg = (torch.rand(H, 2 * H, generator=g, device=dev) * 2 - 1) * lim
    wc = (torch.rand(H, H, generator=g, device=dev) * 2 - 1) * lim
    mask = torch.arange(T, device=dev)[None, :] < lens[:, None]
    att = torch.softmax(torch.where(mask, rn(B, T) * 3, torch.full((B, T), -1e30, device=dev)), -1)
    go, gh = rn(B, T, H), rn(B, H)

    res = {"batch": B, "maxlen": T, "hidden": H, "iters": args.iters,
           "valid_steps": int(lens.sum())}
    for cell, a in (("gru", None), ("augru", att)):
        out, hf, saved = ops.gru_seq_forward(xp, wg, wc, lens, a)
        res[cell + "_forward_ms"] = round(timed(
            lambda: ops.gru_seq_forward(xp, wg, wc, lens, a), args.iters), 4)
        res[cell + "_backward_ms"] = round(timed(
            lambda: ops.gru_seq_backward(wg, wc, lens, a, out, saved, go, gh), args.iters), 4)
        if args.no_torch:
            continue
        leaves = [t.clone().requires_grad_(True) for t in (xp, wg, wc)]
        al = None if a is None else a.clone().requires_grad_(True)

        def torch_arm():
            o, h = ops._gru_sequence_torch(leaves[0], leaves[1], leaves[2], lens, al)
            ((o * go).sum() + (h * gh).sum()).backward()
            return o, h

        def native_arm():
            o, h = ops._GruSequenceFn.apply(leaves[0], leaves[1], leaves[2], lens, al)
            ((o * go).sum() + (h * gh).sum()).backward()
            return o, h

        grads = {}
        for name, arm in (("torch", torch_arm), ("native", native_arm)):
            for t in leaves + ([al] if al is not None else []):
                t.grad = None
            o, h = arm()
            grads[name] = [o.detach(), h.detach()] + [t.grad.clone() for t in leaves] + (
                [al.grad.clone()] if al is not None else [])
        res[cell + "_arms_max_abs_diff"] = [float((x - y).abs().max())
                                            for x, y in zip(grads["torch"], grads["native"])]
        n = max(2, args.iters // 4)
        res[cell + "_torch_fwd_bwd_ms"] = round(timed(torch_arm, n, warmup=1), 3)
        res[cell + "_native_fwd_bwd_ms"] = round(timed(native_arm, n, warmup=1), 3)
    dr.status_check(dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
