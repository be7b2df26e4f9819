#!/usr/bin/env python3
"""Time the reconstruction term of one training step with and without its gradient to feats on the MI355X (forward plus backward) at
the training shape - B = 32, D = 70, C = 384, 28 x 28 - one JSON line per form into profiles/rec_feats_time.jsonl:

    torch_feats  conv2d, two F.normalize, product, sum, mean, autograd (float32) with feats.requires_grad: what a user had for this
                 gradient without the fused route
    fused        rec_loss.reconstruction_loss on a feats that does not ask: k_rec_bwd_code<false>, the route as it was
    fused_feats  reconstruction_loss(feats_grad=True) on a feats that asks: k_rec_bwd_code<true> stores d feats (B,C,h,w) as well

Host clock around `--steps` calls ending in a device synchronise, after warm-up; the forms alternate in one process and each is
repeated `--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per call).  On the fused_feats
line: whether its interval lies below torch_feats', the medians' difference to `fused`, and the time the extra store's bytes take
at `--hbm-tbs` TB/s.  `--only fused_feats --steps N --repeats 1` is the program for a kernel trace.  Needs the GPU.

    python scripts/rec_feats_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/rec_feats_time.jsonl]
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
    ap.add_argument("--only", choices=["torch_feats", "fused", "fused_feats"], default=None)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM rate the extra store is set against, TB/s")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_feats_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rec_feats_time.py: needs the GPU (the fused route has no CPU path)")
    dev = torch.device("cuda:0")
    B, D, C, hw = 32, 70, 384, 28
    g = torch.Generator().manual_seed(0)
    code = (torch.randn(B, D, hw, hw, generator=g) + 0.6).to(dev).requires_grad_(True)
    feats = (torch.randn(B, C, hw, hw, generator=g) + 0.3).to(dev)
    feats_g = feats.clone().requires_grad_(True)
    bound = 1.0 / math.sqrt(D)              # nn.Conv2d's default initialisation
    weight = ((torch.rand(C, D, 1, 1, generator=g) * 2 - 1) * bound).to(dev).requires_grad_(True)
    bias = ((torch.rand(C, generator=g) * 2 - 1) * bound).to(dev).requires_grad_(True)
    last = {}

    def route(name, fn, f):
        def run():
            code.grad = weight.grad = bias.grad = feats_g.grad = None
            loss = fn(code, f, weight, bias)
            loss.backward()
            last[name] = (loss.detach(), code.grad, weight.grad, bias.grad, feats_g.grad)
        return run

    forms = {"torch_feats": route("torch_feats", torch_chain, feats_g),
             "fused": route("fused", reconstruction_loss, feats),
             "fused_feats": route("fused_feats", lambda c, f, w, b: reconstruction_loss(c, f, w, b, feats_grad=True), feats_g)}
    if args.only:
        forms = {args.only: forms[args.only]}
    for f in forms.values():
        clock(f, args.warmup)
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, f in forms.items():
            times[k].append(clock(f, args.steps))
    lines = []
    for k, ts in times.items():
        rec = {"form": k, "shape": f"B={B}, D={D}, C={C}, {hw}x{hw}, forward + backward", "steps": args.steps, **spread(ts)}
        if k == "fused_feats" and len(forms) == 3:
            a, b, c = last["torch_feats"], last["fused"], last["fused_feats"]
            rel = lambda x, y: float((x - y).norm() / x.norm())
            store_bytes = B * C * hw * hw * 4
            rec.update({"faster_than_torch_feats_with_disjoint_intervals": bool(max(ts) < min(times["torch_feats"])),
                        "vs_torch_feats": round(statistics.median(ts) / statistics.median(times["torch_feats"]), 5),
                        "us_over_fused": round(statistics.median(ts) - statistics.median(times["fused"]), 2),
                        "extra_store_bytes": store_bytes, "hbm_tbs": args.hbm_tbs,
                        "us_extra_store_at_hbm_rate": round(store_bytes / (args.hbm_tbs * 1e12) * 1e6, 2),
                        "d_feats_rel_l2_between_forms": rel(a[4], c[4]), "d_code_rel_l2_between_forms": rel(a[1], c[1]),
                        "d_code_bits_equal_to_fused": bool(torch.equal(b[1], c[1])), "d_weight_bits_equal_to_fused": bool(torch.equal(b[2], c[2]))})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
