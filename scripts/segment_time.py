#!/usr/bin/env python3
"""Time label-free inference behind the featurizer at the evaluation shape scripts/eval_time.py uses - B = 8, D = 70, 40 x 40 code to
320 x 320 pixels, 27 classes + 27 clusters, with the flipped pass - one JSON line per form into profiles/segment_time.jsonl:

    torch_chain   the reference's order with torch ops on the same GPU (src/demo_segmentation.py:59-78 without the CRF, and the lookups
                  of src/eval_segmentation.py:170-240): average the two codes, F.interpolate, 1 x 1 convolution and normalised
                  inner products at 320 x 320, two arg-maxes, the cluster table lookup, uint8 casts, two colour lookups
    segment       evaluation.segment writing the same four outputs (dg_segment_labels: two launches)

Host clock around `--steps` calls ending in a device synchronise, after warm-up; the forms alternate in one process and each is
repeated `--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per call), and whether the fused
form's interval lies below the torch chain's.  `--only FORM --steps N --repeats 1` is the program for a kernel trace.  Needs the GPU.

    python scripts/segment_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/segment_time.jsonl]
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

from depthg_amd import ops, segment  # noqa: E402
from depthg_amd.head import ClusterLookup  # noqa: E402

B, D, h, w, H, W, N, M = 8, 70, 40, 40, 320, 320, 27, 27


def clock(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def spread(ts):
    return {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2), "repeats": len(ts)}


class Assignment:
    """An UnsupervisedMetrics stand-in whose compute() has run: a fixed permutation."""

    def __init__(self, table):
        self.assignments, self.table = (None, table.numpy()), table

    def map_clusters(self, clusters):
        return self.table[clusters]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["torch_chain", "segment"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segment_time.py: needs the GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    code, code_flip = torch.randn(B, D, h, w, generator=g).to(dev), torch.randn(B, D, h, w, generator=g).to(dev)
    linear, cluster = torch.nn.Conv2d(D, N, (1, 1)).to(dev), ClusterLookup(D, M).to(dev)
    table = torch.randperm(M, generator=g)
    table_dev, cmap = table.to(dev), ops.pascal_colormap().to(dev)
    metric = Assignment(table)

    def torch_chain():
        with torch.no_grad():
            c = (code + code_flip.flip(dims=[3])) / 2
            up = F.interpolate(c, (H, W), mode="bilinear", align_corners=False)
            lin = linear(up).argmax(1)
            clu = torch.einsum("bchw,nc->bnhw", F.normalize(up, dim=1), F.normalize(cluster.clusters, dim=1)).argmax(1)
            clu = table_dev[clu]
            return lin.to(torch.uint8), clu.to(torch.uint8), cmap[lin], cmap[clu]

    def fused():
        s = segment(code, (H, W), linear, cluster, code_flip=code_flip, cluster_metrics=metric, overlay=1.0)
        return s.linear, s.cluster, s.linear_rgb, s.cluster_rgb

    forms = {"torch_chain": torch_chain, "segment": fused}
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
        rec = {"form": k, "shape": f"B={B}, D={D}, {h}x{w} -> {H}x{W}, n={N}, m={M}, flip, labels + remap + two colour images",
               "steps": args.steps, **spread(ts)}
        if len(forms) == 2:
            rec["vs_torch_chain"] = round(statistics.median(ts) / statistics.median(times["torch_chain"]), 4)
            rec["segment_faster_with_disjoint_intervals"] = bool(max(times["segment"]) < min(times["torch_chain"]))
            a, b = torch_chain(), fused()
            rec["differing_label_pixels"] = int((a[0] != b[0]).sum()) + int((a[1] != b[1]).sum())
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
