"""Time the feature-aware farthest point sampling (cfg.dg_fps_feats) at the headline shape: B = 32 + 32 maps, a 28 x 28 grid, C = 384,
S = 11, depth 224 x 224.  Host clock around 20 calls, five alternated repeats per form, median [min, max] in microseconds per call:
    (a) ops.fps_coords_pair          the depth-only sampler the mode runs without the key
    (b) a torch-on-device restatement of the combined loop: per round one broadcast subtraction, two reductions and an arg-max,
        batched over the 64 images
    (c) ops.fps_feats_coords_pair    the new op
Appends one JSON line per form to profiles/fps_feats_time.jsonl.

    python scripts/fps_feats_time.py [--out profiles/fps_feats_time.jsonl]"""
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
from depthg_amd import ops  # noqa: E402

B, C, HW, S, DEPTH, CALLS, REPEATS = 32, 384, 28, 11, 224, 20, 5


def torch_loop(depth, feats, S):
    """The combined loop in torch on the device, batched over images (selection indices (N, S*S)); the 0 / 0 rule as the library's."""
    N, C, h, w = feats.shape
    d = F.adaptive_avg_pool2d(depth, (h, w))[:, 0]
    factor = 2.0 * torch.tan(torch.tensor([90.0], device=depth.device) / 2.0)
    ys, xs = torch.arange(h, device=depth.device).view(h, 1), torch.arange(w, device=depth.device).view(1, w)
    pts = torch.stack([factor * d * (xs - w / 2.0) / w, factor * d * (ys - h / 2.0) / h, -d * 5.0], -1).reshape(N, h * w, 3)
    f = feats.permute(0, 2, 3, 1).reshape(N, h * w, C)
    rows = torch.arange(N, device=depth.device)
    left = torch.ones(N, h * w, dtype=torch.bool, device=depth.device)
    left[:, 0] = False
    dists = torch.full((N, h * w), float("inf"), device=depth.device)
    last = torch.zeros(N, dtype=torch.long, device=depth.device)
    order = [last]
    for _ in range(1, S * S):
        pd = ((pts[rows, last][:, None] - pts) ** 2).sum(-1)
        fd = ((f[rows, last][:, None] - f) ** 2).sum(-1)
        mp = torch.where(left, pd, pd.new_zeros(())).amax(1, keepdim=True)
        mf = torch.where(left, fd, fd.new_zeros(())).amax(1, keepdim=True)
        dd = torch.where(mp > 0, pd / mp, torch.zeros_like(pd)) + torch.where(mf > 0, fd / mf, torch.zeros_like(fd))
        dists = torch.minimum(dists, dd)
        last = torch.where(left, dists, dists.new_full((), -1.0)).argmax(1)
        left[rows, last] = False
        order.append(last)
    return torch.stack(order, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_feats_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    depth, depth_pos = (torch.rand(B, 1, DEPTH, DEPTH, generator=g).to(dev) * 255 + 1 for _ in range(2))
    feats, feats_pos = (torch.randn(B, C, HW, HW, generator=g).to(dev) for _ in range(2))
    both_d, both_f = torch.cat([depth, depth_pos]), torch.cat([feats, feats_pos])
    forms = {"a_fps_coords_pair": lambda: ops.fps_coords_pair(depth, depth_pos, (HW, HW), S),
             "b_torch_loop": lambda: torch_loop(both_d, both_f, S),
             "c_fps_feats_coords_pair": lambda: ops.fps_feats_coords_pair(depth, depth_pos, feats, feats_pos, (HW, HW), S)}
    # the torch loop and the op select the same points wherever float32 summation order cannot flip a round (reported, not asserted)
    _, inds = ops.fps_feats_coords(both_d, both_f, (HW, HW), S, return_inds=True)
    same = float((torch_loop(both_d, both_f, S) == inds.long()).all(1).float().mean())
    times = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / CALLS * 1e6)
    with open(args.out, "a") as fh:
        for name, ts in times.items():
            line = dict(form=name, B=f"{B}+{B}", grid=HW, C=C, S=S, depth=DEPTH, calls=CALLS, repeats=REPEATS,
                        us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1), us_max=round(max(ts), 1),
                        device=torch.cuda.get_device_name(0), images_selecting_as_torch_loop=same)
            print(json.dumps(line))
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
