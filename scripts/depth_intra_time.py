#!/usr/bin/env python3
"""Time the routes to DepthContrastiveCorrelationLoss of one training step on the MI355X (forward plus backward to both code maps
through `loss.total`) at the shipped recipe's shape - B = 32, C = 384, D = 70, 28 x 28, S = 11, 5 negatives, random coordinates - one
JSON line per form into profiles/depth_intra_time.jsonl:

    two_call   what the loss's linearity in the feature correlation offers without the class: ContrastiveCorrelationLoss on the
               depth-augmented maps with the intra weight alone + ContrastiveCorrelationLoss on the plain maps with the inter and neg
               weights alone, one backward through the sum
    plain      one ContrastiveCorrelationLoss call: the floor
    intra      DepthContrastiveCorrelationLoss (dg_corr_forward_intra_feats): one call, one more gathered operand

Host clock around `--steps` calls ending in a device synchronise, after warm-up; the forms alternate in one process and each is
repeated `--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per call), and whether the new
class's interval lies below the two-call route's.  `--only FORM --steps N --repeats 1` is the program for a kernel trace.  Needs the GPU.

    python scripts/depth_intra_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/depth_intra_time.jsonl]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from depthg_amd import ContrastiveCorrelationLoss, DepthContrastiveCorrelationLoss  # noqa: E402
from oracle import depthg_oracle as O  # noqa: E402


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
    ap.add_argument("--only", choices=["two_call", "plain", "intra"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_intra_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_intra_time.py: needs the GPU (the loss has no CPU path)")
    dev = torch.device("cuda:0")
    B, C, D, hw, S, N = 32, 384, 70, 28, 11, 5
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    f, fp, aug, augp = r(B, C, hw, hw), r(B, C, hw, hw), r(B, C, hw, hw), r(B, C, hw, hw)
    code, code_pos = r(B, D, hw, hw).requires_grad_(True), r(B, D, hw, hw).requires_grad_(True)
    cfg = O.default_cfg(feature_samples=S, neg_samples=N, depth_feat_correlation_loss=False, dg_outputs="reduced", depth_sampling="none",
                        pos_intra_shift=0.18, pos_inter_shift=0.12, neg_inter_shift=0.46)
    cfg_a, cfg_b = copy.copy(cfg), copy.copy(cfg)
    cfg_a.pos_inter_weight = cfg_a.neg_inter_weight = 0.0
    cfg_b.pos_intra_weight = 0.0
    plain, la, lb, intra = (ContrastiveCorrelationLoss(cfg), ContrastiveCorrelationLoss(cfg_a), ContrastiveCorrelationLoss(cfg_b),
                            DepthContrastiveCorrelationLoss(cfg))

    def two_call():
        code.grad = code_pos.grad = None
        la(aug, augp, None, None, code, code_pos)
        lb(f, fp, None, None, code, code_pos)
        (la.total + lb.total).backward()

    def one_plain():
        code.grad = code_pos.grad = None
        plain(f, fp, None, None, code, code_pos)
        plain.total.backward()

    def one_intra():
        code.grad = code_pos.grad = None
        intra(f, fp, None, None, code, code_pos, aug, augp)
        intra.total.backward()

    forms = {"two_call": two_call, "plain": one_plain, "intra": one_intra}
    if args.only:
        forms = {args.only: forms[args.only]}
    for fn in forms.values():
        clock(fn, args.warmup)
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, fn in forms.items():
            times[k].append(clock(fn, args.steps))
    lines = []
    for k, ts in times.items():
        rec = {"form": k, "shape": f"B={B}, C={C}, D={D}, {hw}x{hw}, S={S}, n_neg={N}, random coordinates, forward + backward",
               "steps": args.steps, **spread(ts)}
        if len(forms) == 3:
            rec["vs_plain"] = round(statistics.median(ts) / statistics.median(times["plain"]), 4)
            rec["intra_faster_than_two_call_with_disjoint_intervals"] = bool(max(times["intra"]) < min(times["two_call"]))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
