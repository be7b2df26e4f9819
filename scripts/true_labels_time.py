"""Time what cfg.use_true_labels adds to a step at the headline batch: B = 32 + 32 label maps of 224 x 224, K = n_classes + 1 = 28.
Host clock around 20 calls, five alternated repeats per form, median [min, max] in microseconds per call:
    (a) the reference's torch chain on the device for both maps: F.one_hot(label + 1, K).permute(0, 3, 1, 2).float(), twice
    (b) ops.label_onehot(label, n_classes, label_pos): one launch, both maps
    (c) ops.fps_coords_large_pair at the labels' resolution (224 x 224, S = 11) - 121 sequential rounds over 50 176 points per image
    (d) ops.fps_coords_pair on the 28 x 28 grid of the unsupervised step, for scale
(b) is also stated as bytes moved per second (labels read once, the signal written once).
Appends one JSON line per form to profiles/true_labels_time.jsonl.

    python scripts/true_labels_time.py [--out profiles/true_labels_time.jsonl]"""
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

B, N_CLASSES, HW, S, GRID, CALLS, REPEATS = 32, 27, 224, 11, 28, 20, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_labels_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    label, label_pos = (torch.randint(-1, N_CLASSES, (B, HW, HW), generator=g).to(dev) for _ in range(2))
    depth, depth_pos = (torch.rand(B, 1, HW, HW, generator=g).to(dev) * 255 + 1 for _ in range(2))
    K = N_CLASSES + 1
    chain = lambda t: F.one_hot(t + 1, K).permute(0, 3, 1, 2).to(torch.float32)
    forms = {"a_torch_chain_both_maps": lambda: (chain(label), chain(label_pos)),
             "b_label_onehot_pair": lambda: ops.label_onehot(label, N_CLASSES, label_pos, check=False),
             "c_fps_coords_large_pair_224": lambda: ops.fps_coords_large_pair(depth, depth_pos, (HW, HW), S),
             "d_fps_coords_pair_28": lambda: ops.fps_coords_pair(depth, depth_pos, (GRID, GRID), S)}
    a, b = forms["a_torch_chain_both_maps"](), forms["b_label_onehot_pair"]()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    del a, b
    onehot_bytes = 2 * B * HW * HW * (8 + 4 * K)
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
            line = dict(form=name, B=f"{B}+{B}", K=K, label_hw=HW, S=S, calls=CALLS, repeats=REPEATS, us_median=round(statistics.median(ts), 1),
                        us_min=round(min(ts), 1), us_max=round(max(ts), 1), device=torch.cuda.get_device_name(0))
            if name == "b_label_onehot_pair":
                line.update(bytes=onehot_bytes, tb_per_s_at_median=round(onehot_bytes / statistics.median(ts) / 1e6, 3))
            print(json.dumps(line))
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
