#!/usr/bin/env python3
"""Time the two routes to the cd histograms of one loss call on the MI355X, at the headline shape (B = 32, C = 384, D = 70, 28 x 28
maps on the dense identity grid, 5 negatives, after a gradient forward), one JSON line per form into profiles/cd_hist_time.jsonl:

    materialize_histc   the only route before dg_corr_cd_hist: seven ops.corr_materialize calls for the un-reduced cd tensors
                        ((B,28,28,28,28) fp32, 78.7 MB each) and torch.histc on each
    cd_histograms       ContrastiveCorrelationLoss.cd_histograms(): one memset node + one k_cd_hist launch on the operands the
                        forward left in its workspace

Host clock around `--steps` calls ending in a device synchronise, after warm-up; the two forms alternate and each is repeated
`--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per call), and whether the two intervals
are disjoint.  Needs the GPU.

    python scripts/cd_hist_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/cd_hist_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from depthg_amd import ContrastiveCorrelationLoss, ops  # noqa: E402
from depthg_amd.segmenter import default_segmenter_cfg  # noqa: E402


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
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cd_hist_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cd_hist_time.py: needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    B, C, D, S, N = 32, 384, 70, 28, 5
    g = torch.Generator().manual_seed(0)
    feats, feats_pos = (torch.randn(B, C, S, S, generator=g).to(dev) for _ in range(2))
    code, code_pos = (torch.randn(B, D, S, S, generator=g).to(dev).requires_grad_(True) for _ in range(2))
    depth, depth_pos = (torch.randint(1, 256, (B, 1, 8 * S, 8 * S), generator=g).float().to(dev) for _ in range(2))
    cfg = default_segmenter_cfg(dim=D, feature_samples=S, neg_samples=N, depth_sampling="none", dg_dense_grid=True, dg_outputs="reduced")
    loss = ContrastiveCorrelationLoss(cfg)
    torch.manual_seed(1)
    loss(feats, feats_pos, None, None, code, code_pos, depth, depth_pos)          # a gradient forward: the operands stay in its workspace
    desc, perms, ws = loss.last_call
    assert desc.flags & ops._lib.DG_IDENTITY_GRID and desc.flags & ops._lib.DG_NEED_GRAD
    bins = args.bins

    def materialize_histc():
        hs = [torch.histc(ops.corr_materialize(desc, t, ws, perms=perms)[0], bins=bins, min=-1.0, max=1.0) for t in range(2 + N)]
        return {"intra_cd": hs[0], "inter_cd": hs[1], "neg_cd": torch.stack(hs[2:]).sum(0)}

    forms = {"materialize_histc": materialize_histc, "cd_histograms": lambda: loss.cd_histograms(bins=bins)}
    a, b = forms["materialize_histc"](), forms["cd_histograms"]()
    numel = B * (S * S) ** 2
    # (histc drops what rounding pushed past +-1 and bins fp32 values of another kernel: the two forms agree up to elements at an edge)
    moved = {k: int((a[k].double() - b[k].double()).abs().sum().item()) // 2 for k in a}
    for fn in forms.values():
        clock(fn, args.warmup)
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, fn in forms.items():
            times[k].append(clock(fn, args.steps))
    base = statistics.median(times["materialize_histc"])
    disjoint = max(times["cd_histograms"]) < min(times["materialize_histc"])
    lines = []
    for k, ts in times.items():
        lines.append(json.dumps({"form": k, "shape": f"B={B}, C={C}, D={D}, {S}x{S} identity grid, {N} negatives, {bins} bins on [-1, 1]",
                                 "elements_per_pair_set": numel, "steps": args.steps, **spread(ts),
                                 "vs_materialize_histc": round(statistics.median(ts) / base, 5),
                                 "faster_with_disjoint_intervals": bool(disjoint),
                                 "elements_binned_differently_between_forms": moved}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
