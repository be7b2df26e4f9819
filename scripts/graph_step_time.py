"""Times an epoch of cached training through the host-chosen route against the recorded one.

    python scripts/graph_step_time.py [--out profiles/graph_step_time.jsonl] [--repeats 5] [--epochs 4] [--images 256] [--only a|b|c|bc] [--append]

vit_small(8) with seeded random weights, a float16 feature cache and a sample cache of `--images` stub images (the folder of
scripts/sample_cache_time.py), B = 32, 224 x 224, label and depth.  Two forms in one process, alternated inside each of `--repeats`
repeats, `--epochs` epochs per sample, host clock between two device synchronisations:
    a_contrastive_batches   the parent's route: data.ContrastiveBatches (both caches) + training_step, cfg.dg_fused_adam
    b_graphed_train_step    epoch.DeviceEpoch + graph_step.GraphedTrainStep (cfg.dg_graph_step): begin_epoch() and step() per batch
    c_graphed_fused_probes  (b) with cfg.dg_fused_probes: both probes as one fused operation (only with --only c or --only bc)
One JSON line per form: batches per second, median [min, max] over the repeats, and for (b), (c) the recordings made and the share of
steps that were replays.  --only b runs that form alone (for a kernel trace); --only bc alternates (b) and (c); --append adds the
lines to --out instead of replacing it.
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
    ap.add_argument("--out", default=os.path.join("profiles", "graph_step_time.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--only", choices=("a", "b", "c", "bc"), default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    from depthg_amd import data
    from depthg_amd.epoch import DeviceEpoch
    from depthg_amd.graph_step import GraphedTrainStep
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    dev = torch.device("cuda:0")
    B, res, N = 32, 224, args.images

    def segmenter(**over):
        cfg = default_segmenter_cfg(dg_dino_backbone=True, dg_feature_cache="float16", dg_fused_adam=True, res=res, **over)
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            seg = UnsupervisedSegmenter(27, cfg).to(dev)
        seg.train()
        return seg

    lines = []
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, N)
        ds = data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train", return_depth=True)
        seg_a, seg_b = segmenter(), segmenter(dg_graph_safe=True, dg_graph_step=True)
        cache = data.new_sample_cache(ds, "train", res, "center", True, dev)
        feats = data.build_feature_cache(seg_a.net, ds, seg_a.cfg, res, "center", dtype=torch.float16, device=dev, batch_size=64, num_workers=16,
                                         sample_cache=cache)
        batches = data.ContrastiveBatches(ds, seg_a.cfg, "train", res, "center", B, shuffle=True, generator=torch.Generator().manual_seed(1),
                                          num_workers=16, device=dev, feature_cache=feats, sample_cache=cache)
        epoch = DeviceEpoch(batches.nns, B, batches.num_neighbors, dev, shuffle=True, generator=torch.Generator().manual_seed(1))
        graphed = GraphedTrainStep(seg_b, epoch, cache, feats, label_dims=ds.label_dims)
        replays = [0, 0]
        graphed_c, replays_c = None, [0, 0]
        if args.only and "c" in args.only:
            epoch_c = DeviceEpoch(batches.nns, B, batches.num_neighbors, dev, shuffle=True, generator=torch.Generator().manual_seed(1))
            graphed_c = GraphedTrainStep(segmenter(dg_graph_safe=True, dg_graph_step=True, dg_fused_probes=True), epoch_c, cache, feats,
                                         label_dims=ds.label_dims)

        def form_c():
            for _ in range(args.epochs):
                epoch_c.begin_epoch()
                for _ in range(epoch_c.steps_per_epoch):
                    graphed_c.step()
                    replays_c[0] += int(graphed_c.graphed)
                    replays_c[1] += 1

        def form_a():
            for _ in range(args.epochs):
                for i, batch in enumerate(batches):
                    seg_a.training_step(batch, i)

        def form_b():
            for _ in range(args.epochs):
                epoch.begin_epoch()
                for _ in range(epoch.steps_per_epoch):
                    graphed.step()
                    replays[0] += int(graphed.graphed)
                    replays[1] += 1

        forms = {"a_contrastive_batches": (form_a, len(batches)), "b_graphed_train_step": (form_b, epoch.steps_per_epoch)}
        if graphed_c is not None:
            forms["c_graphed_fused_probes"] = (form_c, epoch.steps_per_epoch)
        if args.only:
            forms = {k: v for k, v in forms.items() if k[0] in args.only}
        for fn, _ in forms.values():                # warm-up: allocator, kernel attributes, clocks, the first recording
            timed(fn)
        replays[:] = [0, 0]
        replays_c[:] = [0, 0]
        samples = {name: [] for name in forms}
        for _ in range(args.repeats):
            for name, (fn, per_epoch) in forms.items():
                samples[name].append(per_epoch * args.epochs / timed(fn))
        for name, rate in samples.items():
            rate = sorted(rate)
            line = {"form": name, "unit": "batches per second", "median": round(statistics.median(rate), 2), "min": round(rate[0], 2),
                    "max": round(rate[-1], 2), "repeats": args.repeats, "epochs_per_sample": args.epochs, "batches_per_epoch": forms[name][1],
                    "images": N, "batch_size": B, "ms_per_batch_at_median": round(1e3 / statistics.median(rate), 4)}
            if name.startswith("b_"):
                line.update({"recordings": graphed.captures, "replayed_steps": replays[0], "timed_steps": replays[1]})
            if name.startswith("c_"):
                line.update({"recordings": graphed_c.captures, "replayed_steps": replays_c[0], "timed_steps": replays_c[1]})
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as out:
        for line in lines:
            line["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
