"""Times the depth encoder of a dino_depth step on the GPU: (a) the torch route (the nn.Sequential under autograd: what
cfg.dg_fused_depth_encoder = False runs) against (b) the fused HIP route (depthg_amd.depth_encoder), forward plus backward of one
encoder pass at the training shape (B = 32, depth 224 x 224, feature grid 28 x 28, n_feats = 384), and a whole `training_step` under
guidance "sum" with and without the flag.  Host clock around CALLS calls between two synchronisations, REPEATS repeats, the forms
alternated inside every repeat; median [min, max] per call.  One JSON line per form -> profiles/depth_encoder_time.jsonl.

    python scripts/depth_encoder_time.py [--out profiles/depth_encoder_time.jsonl] [--calls 20] [--repeats 5] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def alternate(forms, calls, repeats, warmup=3):
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            times[k].append(timed(fn, calls))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "depth_encoder_time.jsonl"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    from depthg_amd import depth_encoder
    from depthg_amd.featurizer import make_depth_downscaling
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    dev = torch.device("cuda:0")
    B, h, w, C = 32, 28, 28, 384
    torch.manual_seed(0)
    stack = make_depth_downscaling(C).to(dev)
    depth = torch.rand(B, 1, 8 * h, 8 * w, device=dev)
    feat = torch.randn(B, C, h, w, device=dev)
    gout = torch.randn(B, C, h, w, device=dev)

    def torch_route():
        stack.zero_grad(set_to_none=True)
        (feat + stack(depth)).backward(gout)

    def fused_route():
        stack.zero_grad(set_to_none=True)
        depth_encoder(depth, stack, feat).backward(gout)

    rows = []
    res = alternate({"torch": torch_route, "fused": fused_route}, a.calls, a.repeats)
    for k, v in res.items():
        rows.append({"what": "encoder forward+backward, one pass", "form": k, "B": B, "grid": [h, w], "C": C, "calls": a.calls,
                     "repeats": a.repeats, **v})
    if not a.no_step:
        g = torch.Generator().manual_seed(0)
        batch = {"img": torch.randn(B, 3, 224, 224, generator=g).to(dev), "img_pos": torch.randn(B, 3, 224, 224, generator=g).to(dev),
                 "label": torch.randint(0, 27, (B, 224, 224), generator=g).to(dev),
                 "depth": torch.rand(B, 1, 224, 224, generator=g).to(dev), "depth_pos": torch.rand(B, 1, 224, 224, generator=g).to(dev)}
        segs = {}
        for name, flag in (("step, flag off", False), ("step, flag on", True)):
            torch.manual_seed(1)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                seg = UnsupervisedSegmenter(27, default_segmenter_cfg(arch="dino_depth", guidance="sum", dg_fused_depth_encoder=flag)).to(dev).train()
            segs[name] = (lambda s=seg: s.training_step(batch))
        res = alternate(segs, max(a.calls // 4, 3), a.repeats, warmup=2)
        for k, v in res.items():
            rows.append({"what": "dino_depth training_step, guidance sum (stand-in backbone)", "form": k, "B": B, **v})
    with open(a.out, "w") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
