"""Time the batch augmentation at B = 32, 3 x 224 x 224 under the default parameter distribution, two forms:
    torch_loop   augment.augment_batch_torch on GPU tensors: the float32 torch chain, one image at a time
    fused        augment.augment_batch: two HIP launches for the batch (dg_augment.hip)
Host clock around 20 calls between synchronisations, five repeats with the forms alternated, median [min, max] per call; one JSON line
per form appended to profiles/gpu_augment_time.jsonl (or --out).  Both forms take the same record, drawn once.

    python scripts/gpu_augment_time.py [--out profiles/gpu_augment_time.jsonl]
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
from depthg_amd import augment as A  # noqa: E402

B, H, W, CALLS, REPEATS = 32, 224, 224, 20, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_augment_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, 3, H, W, generator=g).to(dev)
    params = A.draw_augment_params(B, H, W, g)
    forms = {"torch_loop": lambda: A.augment_batch_torch(img, params), "fused": lambda: A.augment_batch(img, params)}
    for fn in forms.values():                      # warm-up: kernels loaded, allocator filled
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(REPEATS):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / CALLS * 1e3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for name, ts in times.items():
            line = {"form": name, "B": B, "H": H, "W": W, "calls": CALLS, "repeats": REPEATS, "ms_median": statistics.median(ts),
                    "ms_min": min(ts), "ms_max": max(ts), "contrast_images": int((params.ops == A.CONTRAST).any(1).sum()),
                    "blurred_images": int((params.blur_sigma > 0).sum()), "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
