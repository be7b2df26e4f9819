#!/usr/bin/env python3
"""Time the projection head's forward plus backward on the MI355X at the paired training shape - B = 32 + 32, C = 384, D = 70,
28 x 28 - in three forms, one JSON line per form into profiles/head_input_grad_time.jsonl:

    params       ProjectionHead.forward_pair, backward to the six parameters (today's step)
    input_grad   the same with input_grad=True and both feature maps requiring grad: one more launch (k_head_dx) and its weight copies
    torch        a plain-torch fp32 head (conv2d, Dropout2d as a product with the same keep masks, ReLU) with autograd to the
                 parameters and to the features: what a user had without the kernel

Host clock around `--steps` calls ending in a device synchronise, after warm-up; the forms alternate in one process and each is
repeated `--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per call).  The lines also
carry what the input gradient must move and multiply at least: 2 (D + C) C P B flops and the 4 B C P byte store.
`--only input_grad --steps N --repeats 1` is the program for a kernel trace.  Needs the GPU.

    python scripts/head_input_grad_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/head_input_grad_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from depthg_amd.head import ProjectionHead, draw_keep_masks_pair  # noqa: E402


def clock(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def spread(ts):
    return {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2), "repeats": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["params", "input_grad", "torch"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_input_grad_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_input_grad_time.py: needs the GPU (the head has no CPU path)")
    dev = torch.device("cuda:0")
    B, C, D, hw = 32, 384, 70, 28
    P = hw * hw
    g = torch.Generator().manual_seed(0)
    fa, fb = (torch.randn(B, C, hw, hw, generator=g).to(dev) for _ in range(2))
    ua, ub = (torch.randn(B, D, hw, hw, generator=g).to(dev) for _ in range(2))
    torch.manual_seed(0)
    head = ProjectionHead(C, D, "nonlinear").to(dev).train()
    keeps = draw_keep_masks_pair(B, C, dev)
    scale = 1.0 / 0.9
    last = {}

    def fused(input_grad):
        def run():
            head.zero_grad(set_to_none=True)
            a, b = fa.detach().requires_grad_(input_grad), fb.detach().requires_grad_(input_grad)
            (c1, _), (c2, _) = head.forward_pair(a, b, True, keeps, input_grad=input_grad)
            ((c1 * ua).sum() + (c2 * ub).sum()).backward()
            last["input_grad" if input_grad else "params"] = (a.grad, b.grad)
        return run

    def plain():
        head.zero_grad(set_to_none=True)
        grads = []
        loss = 0
        for f, u, half in ((fa, ua, slice(0, B)), (fb, ub, slice(B, 2 * B))):
            x = f.detach().requires_grad_(True)
            k1, k2 = ((k[half] * scale)[:, :, None, None] for k in keeps[:2])
            code = head.cluster1(x * k1) + head.cluster2(x * k2)
            loss = loss + (code * u).sum()
            grads.append(x)
        loss.backward()
        last["torch"] = tuple(x.grad for x in grads)

    forms = {"params": fused(False), "input_grad": fused(True), "torch": plain}
    if args.only:
        forms = {args.only: forms[args.only]}
    for f in forms.values():
        clock(f, args.warmup)
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, f in forms.items():
            times[k].append(clock(f, args.steps))
    extra = {"input_grad_min_flops": 2 * (D + C) * C * P * 2 * B, "input_grad_store_bytes": 4 * 2 * B * C * P}
    if "input_grad" in last and "torch" in last:
        rel = lambda x, y: float((x - y).norm() / y.norm())
        extra["d_image_feat_rel_l2_between_forms"] = max(rel(x, y) for x, y in zip(last["input_grad"], last["torch"]))
    if "params" in times and "input_grad" in times:
        extra["input_grad_adds_us_median"] = round(statistics.median(times["input_grad"]) - statistics.median(times["params"]), 2)
    lines = []
    for k, ts in times.items():
        rec = {"form": k, "shape": f"B={B}+{B}, C={C}, D={D}, {hw}x{hw}, forward + backward", "steps": args.steps, **spread(ts), **extra}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
