"""Times the feature cache's gather against the torch chain it replaces, and a training step with and without the cache.

    python scripts/feature_cache_time.py [--out profiles/feature_cache_time.jsonl] [--calls 20] [--repeats 5]

Host clock around `--calls` calls between two device synchronisations, `--repeats` repeats with the forms alternated inside each
repeat; one JSON line per form with the per-call median [min, max] over the repeats, in microseconds.  B = 32 images + 32 positives,
C = 384, 28 x 28 (vit_small, patch 8, 224 x 224 images).
    a_*   the torch chain on a device cache: two index_select, .float(), cat - indices already on the device; a_host_*: the same chain
          from the CPU index tensors a loader holds (two uploads)
    b_*   FeatureCache.gather from host index lists (its checks and its one index upload included), and b_ops_*: ops.feature_cache_gather
          alone, indices already on the device
    c     training_step of UnsupervisedSegmenter with the DINO ViT (vit_small, seeded random weights), through the backbone
    d, e  the same step from a float32 / float16 cache (cfg.dg_feature_cache)
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

HBM_RATE = 6.29e12      # bytes / s: the measured float4-copy rate of an MI355X (8 TB/s nominal)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def measure(forms, calls, repeats):
    for fn in forms.values():       # warm-up: allocator, kernel attributes, clocks
        timed(fn, 3)
    samples = {name: [] for name in forms}
    for _ in range(repeats):
        for name, fn in forms.items():
            samples[name].append(timed(fn, calls))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "feature_cache_time.jsonl"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    from depthg_amd import FeatureCache, ops
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    dev = torch.device("cuda:0")
    B, C, h, w, N = 32, 384, 28, 28, 512
    L = C * h * w
    g = torch.Generator().manual_seed(0)
    ind, ind_pos = torch.randperm(N, generator=g)[:B], torch.randperm(N, generator=g)[:B]
    forms, extra = {}, {}
    for dtype in (torch.float32, torch.float16):
        name = str(dtype).replace("torch.", "")
        cache = FeatureCache(N, C, h, w, dtype=dtype, device=dev)
        for i in range(0, N, 64):
            cache.put(list(range(i, i + 64)), torch.randn(64, C, h, w, generator=g).to(dev))
        ia, ib = ind.to(dev), ind_pos.to(dev)
        forms["a_" + name] = lambda c=cache, ia=ia, ib=ib: torch.cat([c.data.index_select(0, ia).float(), c.data.index_select(0, ib).float()])
        forms["a_host_" + name] = lambda c=cache: torch.cat([c.data.index_select(0, ind.to(dev)).float(), c.data.index_select(0, ind_pos.to(dev)).float()])
        forms["b_" + name] = lambda c=cache: c.gather(ind, ind_pos)
        forms["b_ops_" + name] = lambda c=cache, ia=ia, ib=ib: ops.feature_cache_gather(c.data, ia, ib)
        moved = 2 * B * L * (cache.data.element_size() + 4)
        extra["b_" + name] = extra["b_ops_" + name] = {"bytes_moved": moved}
        a, b = forms["a_" + name](), forms["b_ops_" + name]()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the kernel and the torch chain disagree"
    samples = measure(forms, args.calls, args.repeats)

    if not args.skip_step:
        hw = 224
        batch = {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
                 "label": torch.randint(0, 27, (B, hw, hw), generator=g).to(dev),
                 "depth": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev),
                 "depth_pos": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev)}
        steps = {}
        for name, dtype in (("c_step_uncached", None), ("d_step_float32_cache", torch.float32), ("e_step_float16_cache", torch.float16)):
            torch.manual_seed(0)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                seg = UnsupervisedSegmenter(27, default_segmenter_cfg(dg_dino_backbone=True, dg_feature_cache=None if dtype is None else str(dtype).replace("torch.", ""))).to(dev)
            seg.train()
            if dtype is not None:
                with torch.no_grad():
                    f, fp = seg.net._backbone(batch["img"])[0], seg.net._backbone(batch["img_pos"])[0]
                cache = FeatureCache(2 * B, C, h, w, dtype=dtype, device=dev)
                cache.put(list(range(B)), f)
                cache.put(list(range(B, 2 * B)), fp)
                # (the gather is part of the cached step's cost: the loader does it per batch)
                steps[name] = lambda seg=seg, cache=cache: seg.training_step(
                    dict(batch, **dict(zip(("image_feat", "image_feat_pos"), cache.gather(list(range(B)), list(range(B, 2 * B)))))), 0)
            else:
                steps[name] = lambda seg=seg: seg.training_step(batch, 0)
        samples.update(measure(steps, args.calls, args.repeats))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for name, xs in samples.items():
            line = {"form": name, "unit": "us per call", "median": round(statistics.median(xs), 2), "min": round(min(xs), 2),
                    "max": round(max(xs), 2), "calls": args.calls, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
            if name in extra:
                line.update(extra[name])
                line["hbm_share_at_median"] = round(extra[name]["bytes_moved"] / (line["median"] * 1e-6) / HBM_RATE, 3)
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
