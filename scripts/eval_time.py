#!/usr/bin/env python3
"""Time the probes' scoring at the evaluation config's shape (res 320, batch 8: code (8, 70, 40, 40), labels 320 x 320, 27 classes,
27 clusters, 5 stored images): the fused evaluation.predict_and_score (dg_segment_predict, two launches) against the reference's
order of operations run with torch on the same GPU (F.interpolate -> 1x1 convolution / F.normalize + einsum -> one-hot -> arg-maxes
-> masked bincounts, src/train_segmentation.py:471-499; the flip form adds the code average and the log-softmaxes of
src/eval_segmentation.py:150-165).  HIP-event timing per call, warm-up, median of the repeats; one JSON line per form.

    python scripts/eval_time.py [--repeats 100] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from depthg_amd import predict_and_score  # noqa: E402
from depthg_amd.head import ClusterLookup  # noqa: E402
from depthg_amd.metrics import UnsupervisedMetrics  # noqa: E402

B, D, h, w, H, W, N, EXTRA, N_STORE = 8, 70, 40, 40, 320, 320, 27, 0, 5


def torch_order(code, code_flip, label, linear, clusters, stats_lin, stats_clu, flip):
    """The reference's chain, torch ops on the GPU (in this script only)."""
    with torch.no_grad():
        if flip:
            code = (code + code_flip.flip(dims=[3])) / 2
        up = F.interpolate(code, label.shape[-2:], mode="bilinear", align_corners=False)
        inner = torch.einsum("bchw,nc->bnhw", F.normalize(up, dim=1), F.normalize(clusters, dim=1))
        if flip:
            lin_preds = torch.log_softmax(linear(up), dim=1).argmax(1)
            clu_preds = torch.log_softmax(inner * 2, dim=1).argmax(1)
        else:
            lin_preds = linear(up).argmax(1)
            clu_preds = F.one_hot(torch.argmax(inner, dim=1), clusters.shape[0]).permute(0, 3, 1, 2).to(torch.float32).argmax(1)
        for preds, stats in ((lin_preds, stats_lin), (clu_preds, stats_clu)):
            actual, p = label.reshape(-1), preds.reshape(-1)
            mask = (actual >= 0) & (actual < N) & (p >= 0) & (p < N)
            rows = stats.shape[0]
            stats += torch.bincount(rows * actual[mask] + p[mask], minlength=N * rows).reshape(N, rows).t()
        return lin_preds[:N_STORE], clu_preds[:N_STORE]


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    code = torch.randn(B, D, h, w, generator=g).to(dev)
    code_flip = torch.randn(B, D, h, w, generator=g).to(dev)
    label = torch.randint(-1, N, (B, H, W), generator=g).to(dev)
    linear = torch.nn.Conv2d(D, N, (1, 1)).to(dev)
    cluster = ClusterLookup(D, N + EXTRA).to(dev)
    lm, cm = UnsupervisedMetrics("test/linear/", N, 0, False), UnsupervisedMetrics("test/cluster/", N, EXTRA, True)
    sl = torch.zeros(N, N, dtype=torch.int64, device=dev)
    sc = torch.zeros(N + EXTRA, N, dtype=torch.int64, device=dev)
    for flip in (False, True):
        cf = code_flip if flip else None
        fused = timed(lambda: predict_and_score(code, label, linear, cluster, lm, cm, code_flip=cf, n_store=N_STORE), args.repeats, args.warmup)
        ref = timed(lambda: torch_order(code, cf, label, linear, cluster.clusters, sl, sc, flip), args.repeats, args.warmup)
        # same predictions on these inputs (a pixel may differ only on a near-tie; report the count)
        lp, cp = predict_and_score(code, label, linear, cluster, code_flip=cf, n_store=N_STORE)
        rl, rc = torch_order(code, cf, label, linear, cluster.clusters, sl.clone(), sc.clone(), flip)
        print(json.dumps({"form": "flip" if flip else "validation", "shape": [B, D, h, w, H, W], "n": N, "m": N + EXTRA,
                          "n_store": N_STORE, "fused_ms": round(fused[0], 4), "fused_min_ms": round(fused[1], 4),
                          "torch_order_ms": round(ref[0], 4), "torch_order_min_ms": round(ref[1], 4),
                          "ratio": round(fused[0] / ref[0], 4),
                          "differing_pixels": int((lp != rl).sum()) + int((cp != rc).sum())}))


if __name__ == "__main__":
    main()
