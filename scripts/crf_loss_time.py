#!/usr/bin/env python3
"""Time the two routes to the contrastive CRF term of one training step on the MI355X (forward plus backward to the code map) at the
reference's shape - B = 32, D = 70, 224 x 224 images, 28 x 28 code, resized to 56 x 56, n = 1000 samples, default scalars - one JSON
line per form into profiles/crf_loss_time.jsonl:

    torch       resize, norm, ContrastiveCRFLoss.forward (the (B,n,n) tensor), .mean(), autograd
    mean_loss   ContrastiveCRFLoss.mean_loss: k_crfl_sample, k_crfl_pair, k_loss_reduce forward, k_crfl_backward

Host clock around `--steps` calls ending in a device synchronise, after warm-up; the two forms alternate in one process and each is
repeated `--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per call), and whether the two
intervals are disjoint.  `--only mean_loss --steps N --repeats 1` is the program for a kernel trace.  Needs the GPU.

    python scripts/crf_loss_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/crf_loss_time.jsonl]
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

from depthg_amd import ContrastiveCRFLoss  # noqa: E402


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
    ap.add_argument("--only", choices=["torch", "mean_loss"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_loss_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crf_loss_time.py: needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    B, D, HW, hw, size, n = 32, 70, 224, 28, 56, 1000
    g = torch.Generator().manual_seed(0)
    img = (torch.randn(B, 3, HW, HW, generator=g) * 1.1).clamp(-2.1, 2.6).to(dev)
    code = torch.randn(B, D, hw, hw, generator=g).to(dev).requires_grad_(True)
    coords = torch.stack([torch.randint(0, size, (n,), generator=g), torch.randint(0, size, (n,), generator=g)]).to(dev)
    fn = ContrastiveCRFLoss(n, .5, .15, .05, 10.0, 3.0, 0.0)
    resize = lambda t: F.interpolate(t, (size, size), mode="bilinear", align_corners=False)
    last = {}

    def torch_route():
        code.grad = None
        loss = fn(resize(img), F.normalize(resize(code), dim=1, eps=1e-10), coords=coords).mean()
        loss.backward()
        last["torch"] = (loss.detach(), code.grad)

    def mean_loss():
        code.grad = None
        loss = fn.mean_loss(img, code, size=size, coords=coords)
        loss.backward()
        last["mean_loss"] = (loss.detach(), code.grad)

    forms = {"torch": torch_route, "mean_loss": mean_loss}
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
        (la, ga), (lb, gb) = last["torch"], last["mean_loss"]
        extra = {"faster_with_disjoint_intervals": bool(max(times["mean_loss"]) < min(times["torch"])),
                 "loss_torch": float(la), "loss_mean_loss": float(lb),
                 "d_code_rel_l2_between_forms": float((ga - gb).norm() / ga.norm())}
        base = statistics.median(times["torch"])
    lines = []
    for k, ts in times.items():
        rec = {"form": k, "shape": f"B={B}, D={D}, {HW}x{HW} images, {hw}x{hw} code, size {size}, n={n}, default scalars, forward + backward",
               "steps": args.steps, **spread(ts)}
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
