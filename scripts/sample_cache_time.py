"""Times a batch from the sample cache against the loader it replaces, and an epoch of cached-feature training with and without it.

    python scripts/sample_cache_time.py [--out profiles/sample_cache_time.jsonl] [--calls 20] [--repeats 5] [--images 256] [--skip-epoch]

Host clock around `--calls` calls between two device synchronisations, `--repeats` repeats with the forms alternated inside each
repeat; one JSON line per form with the per-call median [min, max] over the repeats, in microseconds.  B = 32 images + 32 positives,
500 x 375 sources (JPEG images, PNG labels and depth maps in CroppedDataset's layout, written to a temporary folder) to 224 x 224
with a centre crop, label and depth.
    a_batch_of_decoding   ContrastiveBatches.batch_of without a cache: decoding on 16 threads, packing, upload, dg_batch_prep
    b_prepare_decoded     data.prepare_samples on samples already decoded: packing, upload, dg_batch_prep
    c_cache_gather        SampleCache.gather from host index lists (its checks and its one index upload included)
    d_gather_launch       ops.sample_cache_gather alone, indices already on the device
    e_batch_of_cached     ContrastiveBatches.batch_of with the sample cache (the positives' draw and the dictionary included)
Then, unless --skip-epoch: batches per second over one epoch of ContrastiveBatches + training_step (vit_small(8), seeded random weights,
a float16 feature cache), without and with the sample cache, alternated, `--repeats` epochs each.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np
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


def measure(forms, calls, repeats, warm=3):
    for fn in forms.values():       # warm-up: allocator, kernel attributes, clocks, the page cache
        timed(fn, warm)
    samples = {name: [] for name in forms}
    for _ in range(repeats):
        for name, fn in forms.items():
            samples[name].append(timed(fn, calls))
    return samples


def write_folder(root, n, w=500, h=375, seed=0):
    """CroppedDataset's layout with n smooth images (JPEG codes noise badly: these decode at a photograph's cost), labels and depth."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    base = os.path.join(root, "cropped", "cocostuff27_five_crop_0.5")
    for kind in ("img", "label", "depth"):
        os.makedirs(os.path.join(base, kind, "train"), exist_ok=True)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        f = rng.uniform(0.01, 0.08, (3, 2))
        image = np.stack([127 + 120 * np.sin(f[c, 0] * xx + f[c, 1] * yy + i) for c in range(3)], -1) + rng.normal(0, 6, (h, w, 3))
        Image.fromarray(image.clip(0, 255).astype(np.uint8)).save(os.path.join(base, "img", "train", f"{i}.jpg"), quality=90)
        Image.fromarray(((xx // 50 + yy // 50 + i) % 28).astype(np.uint8)).save(os.path.join(base, "label", "train", f"{i}.png"))
        Image.fromarray(((xx + yy + i) % 256).astype(np.uint8)).save(os.path.join(base, "depth", "train", f"{i}_zoedepth.png"))
    table = (np.arange(n)[:, None] + np.arange(8)[None, :] * 7) % n
    os.makedirs(os.path.join(root, "nns"), exist_ok=True)
    np.savez_compressed(os.path.join(root, "nns", "nns_vit_small_cocostuff27_train_five_224.npz"), nns=table.astype(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sample_cache_time.jsonl"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--skip-epoch", action="store_true")
    args = ap.parse_args()
    from depthg_amd import data, ops
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    dev = torch.device("cuda:0")
    B, res, N = 32, 224, args.images
    lines = []
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, N)
        ds = data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train", return_depth=True)
        cfg = default_segmenter_cfg(dg_dino_backbone=True, dg_feature_cache="float16", res=res)
        plain = data.ContrastiveBatches(ds, cfg, "train", res, "center", B, shuffle=True, generator=torch.Generator().manual_seed(0),
                                        num_workers=16, device=dev)
        inds = list(range(0, 2 * B, 2))
        torch.manual_seed(0)
        samples = plain._decode(inds + [int(plain.nns[i, 1]) for i in inds])
        forms = {"a_batch_of_decoding": lambda: plain.batch_of(inds),
                 "b_prepare_decoded": lambda: data.prepare_samples(ds, samples, res, "center", dev, True)}
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            seg = UnsupervisedSegmenter(27, cfg).to(dev)
        seg.train()
        cache = data.new_sample_cache(ds, "train", res, "center", True, dev)
        if args.skip_epoch:
            data.fill_sample_cache(cache, ds, res, "center", num_workers=16)
            feats = None
        else:                                       # one decoding pass for both caches
            feats = data.build_feature_cache(seg.net, ds, cfg, res, "center", dtype=torch.float16, device=dev, batch_size=64, num_workers=16,
                                             sample_cache=cache)
        cached = data.ContrastiveBatches(ds, cfg, "train", res, "center", B, shuffle=True, generator=torch.Generator().manual_seed(0),
                                         num_workers=16, device=dev, sample_cache=cache)
        pos = [int(plain.nns[i, 1]) for i in inds]
        ia, ib = torch.tensor(inds, device=dev), torch.tensor(pos, device=dev)
        forms["c_cache_gather"] = lambda: cache.gather(inds, pos)
        forms["d_gather_launch"] = lambda: ops.sample_cache_gather(cache.data, True, True, ia, ib, label_offset=-1, fill=-1,
                                                                   mask_rule=ops.BATCH_MASK_BOOL_IGNORED)
        forms["e_batch_of_cached"] = lambda: cached.batch_of(inds)
        want, got = data.prepare_samples(ds, samples, res, "center", dev, True), cache.gather(inds, pos)
        assert all(torch.equal(a, b) for a, b in zip(want, got)), "the cache and dg_batch_prep disagree"
        written = 2 * B * res * res * (3 * 4 + 8 + 1 + 4)
        extra = {"d_gather_launch": {"bytes_moved": written + 2 * B * res * res * 5}, "b_prepare_decoded": {"uploaded_bytes": sum(
            p.size for s in samples for p in s if isinstance(p, np.ndarray))}}
        for name, xs in measure(forms, args.calls, args.repeats).items():
            line = {"form": name, "unit": "us per call", "median": round(statistics.median(xs), 2), "min": round(min(xs), 2),
                    "max": round(max(xs), 2), "calls": args.calls, "repeats": args.repeats, **extra.get(name, {})}
            if "bytes_moved" in line:
                line["hbm_share_at_median"] = round(line["bytes_moved"] / (line["median"] * 1e-6) / HBM_RATE, 3)
            lines.append(line)

        if not args.skip_epoch:
            def epoch(batches):
                def run():
                    for i, batch in enumerate(batches):
                        seg.training_step(batch, i)
                return run
            pipes = {name: data.ContrastiveBatches(ds, cfg, "train", res, "center", B, shuffle=True, generator=torch.Generator().manual_seed(1),
                                                   num_workers=16, device=dev, feature_cache=feats, sample_cache=sc)
                     for name, sc in (("f_epoch_feature_cache", None), ("g_epoch_feature_and_sample_cache", cache))}
            per_epoch = len(pipes["f_epoch_feature_cache"])
            for name, xs in measure({k: epoch(v) for k, v in pipes.items()}, 1, args.repeats, warm=1).items():
                rate = sorted(per_epoch / (x * 1e-6) for x in xs)
                lines.append({"form": name, "unit": "batches per second", "median": round(statistics.median(rate), 2), "min": round(rate[0], 2),
                              "max": round(rate[-1], 2), "epochs": args.repeats, "batches_per_epoch": per_epoch, "images": N, "batch_size": B})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for line in lines:
            line["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
