"""Times one whole validation pass - validation_step over every val batch, then on_validation_epoch_end - through the backbone and
from a validation feature cache, and an epoch of graphed `fit` with a validation every 8 batches, with and without that cache.

    python scripts/val_cache_time.py [--out profiles/val_cache_time.jsonl] [--repeats 5] [--images 256] [--epochs 2] [--skip-fit]

vit_small(8) with seeded random weights (no DINO checkpoint can be fetched here: every figure is on random weights), `--images` stub val
images (the folder of scripts/sample_cache_time.py) at 320 x 320, B = 32.  Four forms in one process, alternated inside each of
`--repeats` repeats, host clock between two device synchronisations:
    a_backbone_materialised   the parent's route: the loader, net(img) with the materialised attention, predict_and_score
    b_backbone_fused          the parent's route with cfg.dg_fused_attention and cfg.dg_fused_linear
    c_val_cache_float32       cfg.dg_val_feature_cache: the loader, image_feat from a float32 cache, the eval-mode head, predict_and_score
    d_val_cache_float16_sc    a float16 cache with the val sample cache on: no decoding either
(a) - (c) decode the images in 16 threads, as the train command does without --sample-cache.  One JSON line per form: seconds per
pass, median [min, max], and for (c), (d) the ratio of (b)'s median to theirs and whether the two intervals are disjoint.  Then (unless
--skip-fit) `--epochs` epochs of train.fit under the graphed step (8 steps of 32 an epoch at 224 x 224, validation behind every 8th
batch over the same val images) with the parent's validation (b's model) and with (d)'s, as training batches per second.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sample_cache_time import write_folder  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "val_cache_time.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    from depthg_amd import data, train
    from depthg_amd.epoch import DeviceEpoch
    from depthg_amd.graph_step import GraphedTrainStep
    from depthg_amd.segmenter import UnsupervisedSegmenter
    dev = torch.device("cuda:0")
    B, eval_res, res, N = 32, 320, 224, args.images

    def segmenter(**over):
        cfg = train.build_cfg({"dg_dino_backbone": True, "batch_size": B, "num_workers": 16, "val_freq": 8, "scalar_log_freq": 10 ** 6, **over})
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            seg = UnsupervisedSegmenter(27, cfg).to(dev)
        seg.train()
        return seg

    lines = []
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, N)
        # (the stub folder has one split; its images serve as the val split here and, for the fit, as the train split too)
        val_set = data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train", return_depth=False)
        fused = dict(dg_fused_attention=True, dg_fused_linear=True)
        seg_a, seg_b = segmenter(), segmenter(**fused)
        seg_c, seg_d = segmenter(dg_val_feature_cache="float32", **fused), segmenter(dg_val_feature_cache="float16", **fused)
        val_samples = data.new_sample_cache(val_set, "val", eval_res, "center", False, dev)
        feats16 = data.build_feature_cache(seg_d.net, val_set, seg_d.cfg, eval_res, "center", dtype=torch.float16, device=dev, batch_size=B,
                                           num_workers=16, sample_cache=val_samples, image_set="val")
        feats32 = data.build_feature_cache(seg_c.net, val_set, seg_c.cfg, eval_res, "center", dtype=torch.float32, device=dev, batch_size=B,
                                           num_workers=16, image_set="val")

        def val_batches(seg, **caches):
            return data.ContrastiveBatches(val_set, seg.cfg, "val", eval_res, "center", B, shuffle=False, num_workers=16, pos=False,
                                           return_depth=False, device=dev, **caches)

        def one_pass(seg, batches):
            def run():
                for i, batch in enumerate(batches):
                    seg.validation_step(batch, i)
                seg.on_validation_epoch_end()
            return run

        forms = {"a_backbone_materialised": one_pass(seg_a, val_batches(seg_a)),
                 "b_backbone_fused": one_pass(seg_b, val_batches(seg_b)),
                 "c_val_cache_float32": one_pass(seg_c, val_batches(seg_c, feature_cache=feats32)),
                 "d_val_cache_float16_sc": one_pass(seg_d, val_batches(seg_d, feature_cache=feats16, sample_cache=val_samples))}
        for fn in forms.values():                    # warm-up: allocator, kernel attributes, clocks
            timed(fn)
        samples = {name: [] for name in forms}
        for _ in range(args.repeats):
            for name, fn in forms.items():
                samples[name].append(timed(fn))
        b_sorted = sorted(samples["b_backbone_fused"])
        for name, secs in samples.items():
            secs = sorted(secs)
            line = {"form": name, "unit": "seconds per validation pass", "median": round(statistics.median(secs), 5), "min": round(secs[0], 5),
                    "max": round(secs[-1], 5), "repeats": args.repeats, "images": N, "batch_size": B, "eval_res": eval_res,
                    "batches": (N + B - 1) // B, "weights": "random (seeded)"}
            if name[0] in "cd":
                line.update({"b_median_over_this_median": round(statistics.median(b_sorted) / statistics.median(secs), 2),
                             "disjoint_from_b": bool(secs[-1] < b_sorted[0])})
            if name[0] == "c":
                line["cache_bytes"] = feats32.nbytes
            if name[0] == "d":
                line.update({"cache_bytes": feats16.nbytes, "sample_cache_bytes": val_samples.nbytes})
            lines.append(line)

        if not args.skip_fit:
            # an epoch of the graphed fit: 8 steps of 32, then a validation over the val images (val_freq = 8 is above a quarter of
            # the epoch, so `fit` validates at the end of every epoch: behind every 8th batch)
            train_set = data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train", return_depth=True)
            graph = dict(dg_feature_cache="float16", dg_fused_adam=True, dg_graph_safe=True, dg_graph_step=True, res=res, **fused)
            seg_p, seg_v = segmenter(**graph), segmenter(dg_val_feature_cache="float16", **graph)
            samples_t = data.new_sample_cache(train_set, "train", res, "center", True, dev)
            feats_t = data.build_feature_cache(seg_p.net, train_set, seg_p.cfg, res, "center", dtype=torch.float16, device=dev, batch_size=64,
                                               num_workers=16, sample_cache=samples_t)
            nns = data.ContrastiveBatches(train_set, seg_p.cfg, "train", res, "center", B, device=dev, feature_cache=feats_t,
                                          sample_cache=samples_t).nns
            out_dir = os.path.join(root, "out")
            fits = {}
            for name, seg, caches in (("fit_graph_step_parent_validation", seg_p, dict(sample_cache=val_samples)),
                                      ("fit_graph_step_val_cache", seg_v, dict(sample_cache=val_samples, feature_cache=feats16))):
                epoch = DeviceEpoch(nns, B, 7, dev, shuffle=True, generator=torch.Generator().manual_seed(1))
                graphed = GraphedTrainStep(seg, epoch, samples_t, feats_t, label_dims=train_set.label_dims)
                batches = val_batches(seg, **caches)

                def run(seg=seg, graphed=graphed, batches=batches, epoch=epoch):
                    seg.cfg.max_steps = args.epochs * epoch.steps_per_epoch
                    return train.fit(seg, None, batches, seg.cfg, out_dir, save_checkpoint=lambda m, p: None, graph_step=graphed)
                fits[name] = (run, graphed, epoch)
            for run, _, _ in fits.values():
                timed(run)                           # warm-up: the recording
            rates = {name: [] for name in fits}
            counts = {}
            for _ in range(args.repeats):
                for name, (run, graphed, epoch) in fits.items():
                    state = {}
                    secs = timed(lambda: state.update(run()))
                    rates[name].append(state["steps"] / secs)
                    counts[name] = (state["steps"], state["validations"], graphed.captures)
            for name, rate in rates.items():
                rate = sorted(rate)
                lines.append({"form": name, "unit": "training batches per second, validations included", "median": round(statistics.median(rate), 2),
                              "min": round(rate[0], 2), "max": round(rate[-1], 2), "repeats": args.repeats, "steps_per_sample": counts[name][0],
                              "validations_per_sample": counts[name][1], "recordings": counts[name][2], "val_images": N, "batch_size": B,
                              "val_sample_cache": True, "weights": "random (seeded)"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for line in lines:
            line["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
