#!/usr/bin/env python3
"""Time the two routes to the reconstruction term of one training step on the MI355X (forward plus backward to code and the decoder)
at the training shape - B = 32, D = 70, C = 384, 28 x 28 - one JSON line per form into profiles/rec_loss_time.jsonl:

    torch    conv2d, two F.normalize, product, sum, mean, autograd (float32): what a user had without the fused route
    fused    rec_loss.reconstruction_loss: k_rec_forward, k_loss_reduce forward; k_rec_bwd_code, k_rec_bwd_w, k_rec_combine backward

Host clock around `--steps` calls ending in a device synchronise, after warm-up; the two forms alternate in one process and each is
repeated `--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per call), and whether the two
intervals are disjoint.  `--only fused --steps N --repeats 1` is the program for a kernel trace.  Needs the GPU.

    python scripts/rec_loss_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/rec_loss_time.jsonl]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from depthg_amd import reconstruction_loss  # noqa: E402


def clock(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def spread(ts):
    return {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2), "repeats": len(ts)}


def torch_chain(code, feats, weight, bias):
    rec_feats = F.conv2d(code, weight, bias)
    return -(F.normalize(rec_feats, dim=1, eps=1e-10) * F.normalize(feats, dim=1, eps=1e-10)).sum(1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["torch", "fused"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_loss_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rec_loss_time.py: needs the GPU (the fused route has no CPU path)")
    dev = torch.device("cuda:0")
    B, D, C, hw = 32, 70, 384, 28
    g = torch.Generator().manual_seed(0)
    code = (torch.randn(B, D, hw, hw, generator=g) + 0.6).to(dev).requires_grad_(True)
    feats = (torch.randn(B, C, hw, hw, generator=g) + 0.3).to(dev)
    bound = 1.0 / math.sqrt(D)              # nn.Conv2d's default initialisation
    weight = ((torch.rand(C, D, 1, 1, generator=g) * 2 - 1) * bound).to(dev).requires_grad_(True)
    bias = ((torch.rand(C, generator=g) * 2 - 1) * bound).to(dev).requires_grad_(True)
    last = {}

    def route(name, fn):
        def run():
            code.grad = weight.grad = bias.grad = None
            loss = fn(code, feats, weight, bias)
            loss.backward()
            last[name] = (loss.detach(), code.grad, weight.grad, bias.grad)
        return run

    forms = {"torch": route("torch", torch_chain), "fused": route("fused", reconstruction_loss)}
    if args.only:
        forms = {args.only: forms[args.only]}
    for f in forms.values():
        clock(f, args.warmup)
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, f in forms.items():
            times[k].append(clock(f, args.steps))
    both = len(forms) == 2
    extra = {}
    if both:
        a, b = last["torch"], last["fused"]
        rel = lambda x, y: float((x - y).norm() / x.norm())
        extra = {"faster_with_disjoint_intervals": bool(max(times["fused"]) < min(times["torch"])),
                 "loss_torch": float(a[0]), "loss_fused": float(b[0]), "d_code_rel_l2_between_forms": rel(a[1], b[1]),
                 "d_weight_rel_l2_between_forms": rel(a[2], b[2]), "d_bias_rel_l2_between_forms": rel(a[3], b[3])}
        base = statistics.median(times["torch"])
    lines = []
    for k, ts in times.items():
        rec = {"form": k, "shape": f"B={B}, D={D}, C={C}, {hw}x{hw}, forward + backward", "steps": args.steps, **spread(ts)}
        if both:
            rec["vs_torch"] = round(statistics.median(ts) / base, 5)
            rec.update(extra)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
