#!/usr/bin/env python3
"""Time the optimisation step's Adams on the MI355X: the segmenter's default parameter set (nine fp32 tensors, 205 547 elements;
src/train_segmentation.py:537-547) with seeded gradients, one JSON line per form:

    torch_adam_x3          three torch.optim.Adam as configure_optimizers() returns them without cfg.dg_fused_adam (the parent form)
    torch_adam_fused_x3    the same three with torch's own fused=True (three launches)
    fused_adam_set         optim.FusedAdamSet, eager (one launch, host step count)
    fused_adam_set_graph   optim.FusedAdamSet over capturable members, replayed from a torch.cuda.graph (device step count)
    training_step          whole training_steps at the headline+head shapes (B = 32, 224 x 224 images -> 28 x 28 dense grid, dim 70)
                           with cfg.dg_fused_adam off and on

Host clock around `--steps` steps ending in a device synchronise, after warm-up; the forms alternate and each is repeated
`--repeats` times: median, minimum and maximum of the repeats are on the line (microseconds per step).  Needs the GPU.

    python scripts/adam_time.py [--steps 2000] [--repeats 5] [--warmup 200] [--train-steps 60]
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

from depthg_amd.optim import FusedAdam, FusedAdamSet  # noqa: E402
from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg  # noqa: E402


def clock(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def spread(ts):
    return {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2), "repeats": len(ts)}


def optimiser_forms(dev, args):
    torch.manual_seed(0)
    forms = {}

    def model():
        torch.manual_seed(1)
        m = UnsupervisedSegmenter(27, default_segmenter_cfg()).to(dev)
        g = torch.Generator().manual_seed(2)
        for p in m.all_reduced_parameters():
            p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to(dev)
        return m

    m = model()
    o = m.configure_optimizers()
    forms["torch_adam_x3"] = lambda o=o: (o[0].step(), o[2].step(), o[1].step())
    m2 = model()
    o2 = (torch.optim.Adam(m2.head_parameters(), lr=m2.cfg.lr, fused=True), torch.optim.Adam(list(m2.linear_probe.parameters()), lr=5e-3, fused=True),
          torch.optim.Adam(list(m2.cluster_probe.parameters()), lr=5e-3, fused=True))
    forms["torch_adam_fused_x3"] = lambda o=o2: (o[0].step(), o[2].step(), o[1].step())
    m3 = model()
    m3.cfg.dg_fused_adam = True
    s3 = FusedAdamSet(m3.configure_optimizers())
    forms["fused_adam_set"] = s3.step
    m4 = model()
    s4 = FusedAdamSet([FusedAdam(m4.head_parameters(), lr=m4.cfg.lr, capturable=True),
                       FusedAdam(list(m4.linear_probe.parameters()), lr=5e-3, capturable=True),
                       FusedAdam(list(m4.cluster_probe.parameters()), lr=5e-3, capturable=True)])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s4.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            s4.step()
    torch.cuda.synchronize()
    forms["fused_adam_set_graph"] = graph.replay
    keep = (m, m2, m3, m4, graph)                       # noqa: F841  (alive while the forms run)
    for fn in forms.values():
        clock(fn, args.warmup)
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, fn in forms.items():
            times[k].append(clock(fn, args.steps))
    base = statistics.median(times["torch_adam_x3"])
    for k, ts in times.items():
        print(json.dumps({"form": k, "elements": 205_547, "tensors": 9, "steps": args.steps, **spread(ts),
                          "vs_torch_adam_x3": round(statistics.median(ts) / base, 4)}), flush=True)
    assert float(s4.optimisers[0].state[m4.head_parameters()[0]]["step"]) == 1 + args.warmup + args.repeats * args.steps


def training_forms(dev, args):
    g = torch.Generator().manual_seed(3)
    B, hw = 32, 224
    batch = {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
             "label": torch.randint(-1, 27, (B, hw, hw), generator=g).to(dev),
             "depth": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev),
             "depth_pos": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev)}
    models = {}
    for flag in (False, True):
        torch.manual_seed(4)
        cfg = default_segmenter_cfg(dim=70, dropout=True, feature_samples=28, depth_sampling="none", dg_dense_grid=True, dg_outputs="reduced",
                                    fps_sample_decay=False, depth_loss_decay=False, dg_fused_adam=flag)
        m = UnsupervisedSegmenter(27, cfg).to(dev)
        m.train()
        models[flag] = m
    forms = {("training_step_fused_adam" if flag else "training_step_torch_adam"): (lambda m=m: m.training_step(batch, 0)) for flag, m in models.items()}
    for fn in forms.values():
        clock(fn, 10)
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, fn in forms.items():
            times[k].append(clock(fn, args.train_steps))
    base = statistics.median(times["training_step_torch_adam"])
    for k, ts in times.items():
        print(json.dumps({"form": k, "shape": "B=32, 224x224 -> 28x28 dense grid, C=384, dim=70 (headline+head), stand-in backbone included",
                          "steps": args.train_steps, **spread(ts), "vs_torch_adam": round(statistics.median(ts) / base, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--train-steps", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adam_time.py: needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    optimiser_forms(dev, args)
    training_forms(dev, args)


if __name__ == "__main__":
    main()
