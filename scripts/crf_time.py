#!/usr/bin/env python3
"""Time the dense-CRF refinement of the evaluation at the eval config's shape (res 320, batch 8: code (8, 70, 40, 40) and its
mirror pass, labels and images 320 x 320, 27 classes, 27 clusters, MAX_ITER = 10):
  run_crf     evaluation.predict_and_score(..., run_crf=True): eval-route unary of both probes, one mean-field call on 27 + 27
              channels, both confusion updates (src/eval_segmentation.py:146-170 with run_crf)
  dense_crf   ops.dense_crf alone on the same unary (predictions only)
Beside them, for context only, the time per image of the numpy restatement the tests compare against (tests/crf_reference.py), on
the host.  The images are normalised random uint8 images: every pixel has its own colour, the largest lattices there are.
HIP-event timing per call, warm-up, median of the repeats; one JSON line per form.

    python scripts/crf_time.py [--repeats 10] [--warmup 2] [--no-cpu]
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

from depthg_amd import crf, ops, predict_and_score  # noqa: E402
from depthg_amd.head import ClusterLookup  # noqa: E402
from depthg_amd.metrics import UnsupervisedMetrics  # noqa: E402

B, D, h, w, H, W, N, EXTRA = 8, 70, 40, 40, 320, 320, 27, 0


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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host restatement's time")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    code = torch.randn(B, D, h, w, generator=g).to(dev)
    code_flip = torch.randn(B, D, h, w, generator=g).to(dev)
    label = torch.randint(-1, N, (B, H, W), generator=g).to(dev)
    u8 = torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255
    img = ((u8 - torch.tensor([0.485, 0.456, 0.406])[:, None, None]) / torch.tensor([0.229, 0.224, 0.225])[:, None, None]).to(dev)
    linear = torch.nn.Conv2d(D, N, (1, 1)).to(dev)
    cluster = ClusterLookup(D, N + EXTRA).to(dev)
    lm, cm = UnsupervisedMetrics("final/linear/", N, 0, False), UnsupervisedMetrics("final/cluster/", N, EXTRA, True)
    med, mn = timed(lambda: predict_and_score(code, label, linear, cluster, lm, cm, code_flip=code_flip, n_store=B, img=img,
                                              run_crf=True), args.repeats, args.warmup)
    print(json.dumps({"form": "run_crf", "shape": [B, D, h, w, H, W], "n": N, "m": N + EXTRA, "flip": True,
                      "n_iter": crf.MAX_ITER, "ms": round(med, 3), "min_ms": round(mn, 3), "ms_per_image": round(med / B, 3)}),
          flush=True)
    with torch.no_grad():
        U = ops.segment_unary(code, linear.weight, linear.bias, cluster.clusters, H, W, code_flip=code_flip)
    ends = [N, 2 * N + EXTRA]
    kw = dict(n_iter=crf.MAX_ITER, pos_w=crf.POS_W, pos_xy_std=crf.POS_XY_STD, bi_w=crf.Bi_W, bi_xy_std=crf.Bi_XY_STD,
              bi_rgb_std=crf.Bi_RGB_STD, return_q=False, return_preds=True)
    med, mn = timed(lambda: ops.dense_crf(img, U, ends, **kw), args.repeats, args.warmup)
    print(json.dumps({"form": "dense_crf", "shape": [B, ends[-1], H, W], "groups": ends, "n_iter": crf.MAX_ITER,
                      "ms": round(med, 3), "min_ms": round(mn, 3), "ms_per_image": round(med / B, 3)}), flush=True)
    if not args.no_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import crf_reference as R
        t0 = time.perf_counter()
        R.dense_crf(img[0].cpu().numpy(), U[0].cpu().numpy(), ends)
        print(json.dumps({"form": "cpu_restatement", "shape": [1, ends[-1], H, W], "n_iter": crf.MAX_ITER,
                          "ms_per_image": round((time.perf_counter() - t0) * 1e3, 1), "note": "numpy on the host; context only"}),
              flush=True)


if __name__ == "__main__":
    main()
