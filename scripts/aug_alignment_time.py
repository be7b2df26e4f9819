#!/usr/bin/env python3
"""Time the two routes to the augmentation-alignment term of one training step on the MI355X (forward plus backward to both code maps)
at the reference's shape - B = 32, D = 70, 28 x 28 code and code_aug, a 224 x 224 coordinate map from crop_flip_coords - one JSON line
per form into profiles/aug_alignment_time.jsonl:

    torch    resize, permutes, grid_sample, two F.normalize, einsum, mean, autograd (float32)
    fused    aug_loss.aug_alignment_loss: k_aug_forward, k_loss_reduce forward; k_aug_bwd_pos, k_aug_taps, k_aug_gather backward

Host clock around `--steps` calls ending in a device synchronise, after warm-up; the two forms alternate in one process and each is
repeated `--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per call), and whether the two
intervals are disjoint.  `--only fused --steps N --repeats 1` is the program for a kernel trace.  Needs the GPU.

    python scripts/aug_alignment_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/aug_alignment_time.jsonl]
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

from depthg_amd import aug_alignment_loss, crop_flip_coords  # noqa: E402


def clock(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def spread(ts):
    return {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2), "repeats": len(ts)}


def torch_chain(code, code_aug, coord_aug):
    n = code_aug.shape[2]
    ds = F.interpolate(coord_aug.permute(0, 3, 1, 2), (n, n), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    u = F.grid_sample(code, ds.permute(0, 2, 1, 3), padding_mode="border", align_corners=True)
    return -torch.einsum("bkhw,bkhw->bhw", F.normalize(u, dim=1, eps=1e-10), F.normalize(code_aug, dim=1, eps=1e-10)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["torch", "fused"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_alignment_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aug_alignment_time.py: needs the GPU (the fused route has no CPU path)")
    dev = torch.device("cuda:0")
    B, D, hw, HW = 32, 70, 28, 224
    g = torch.Generator().manual_seed(0)
    code = (torch.randn(B, D, hw, hw, generator=g) + 0.6).to(dev).requires_grad_(True)
    code_aug = (torch.randn(B, D, hw, hw, generator=g) + 0.6).to(dev).requires_grad_(True)
    boxes = []
    for _ in range(B):                      # RandomResizedCrop's scale (0.8, 1.0) at aspect 1, every other image flipped
        side = HW * math.sqrt(0.8 + 0.2 * float(torch.rand((), generator=g)))
        boxes.append((float(torch.rand((), generator=g)) * (HW - side), float(torch.rand((), generator=g)) * (HW - side), side, side))
    coord_aug = crop_flip_coords(B, HW, HW, boxes, [b % 2 == 1 for b in range(B)]).to(dev)
    last = {}

    def route(name, fn):
        def run():
            code.grad = None
            code_aug.grad = None
            loss = fn(code, code_aug, coord_aug)
            loss.backward()
            last[name] = (loss.detach(), code.grad, code_aug.grad)
        return run

    forms = {"torch": route("torch", torch_chain), "fused": route("fused", aug_alignment_loss)}
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
        (la, ga, ha), (lb, gb, hb) = last["torch"], last["fused"]
        extra = {"faster_with_disjoint_intervals": bool(max(times["fused"]) < min(times["torch"])),
                 "loss_torch": float(la), "loss_fused": float(lb),
                 "d_code_rel_l2_between_forms": float((ga - gb).norm() / ga.norm()),
                 "d_code_aug_rel_l2_between_forms": float((ha - hb).norm() / ha.norm())}
        base = statistics.median(times["torch"])
    lines = []
    for k, ts in times.items():
        rec = {"form": k, "shape": f"B={B}, D={D}, {hw}x{hw} code and code_aug, {HW}x{HW} coord_aug (crop and flip), forward + backward",
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
