"""Digests of three training steps per configuration of a fixed matrix: what a refactor of the step must leave as it is.

    python scripts/step_equivalence.py [--tree DIR] [--out profiles/step_stages.jsonl] [--values FILE.pt] [--only NAME ...] [--deterministic]
    python scripts/step_equivalence.py --compare A.pt B.pt

For each configuration: torch seeded, UnsupervisedSegmenter with the stand-in backbone, three `training_step`s on one synthetic batch
(B = 2, 3 x 64 x 64, patch 8 -> an 8 x 8 grid, dim 16, 5 classes, feature_samples 5, neg_samples 2, crf_samples 64; depth and labels
at image size).  One JSON line each with SHA-256 digests of the three losses' bytes, of every log entry of every step (keys sorted),
of every parameter after the steps and of torch's CPU and GPU generator states after the steps - the generator states pin the number
and order of the draws.  `--tree`: the checkout whose depthg_amd is imported (default: this one), so that two commits are compared by
one script.  `--values` keeps the digested tensors; `--compare` prints, per configuration and quantity, the largest absolute
difference between two such files (for a configuration whose digests differ between two runs of the same commit).  `--deterministic`
asks torch for deterministic convolution algorithms (its own convolutions' backward otherwise adds with atomics).
"""
import argparse
import hashlib
import json
import os
import sys

import torch

B, HW, N_CLASSES = 2, 64, 5
BASE = dict(dim=16, feature_samples=5, neg_samples=2, crf_samples=64, res=HW)
DEPTH = dict(arch="dino_depth", guidance="sum")
# name -> (cfg overrides, batch extras: "feats" = image_feat / image_feat_pos, "aug" = img_aug / coord_aug, "bucket" = grad_sync hands a GradBucket)
MATRIX = {
    "pair": ({}, ()),
    "pair_deferred": (dict(feature_samples=8, depth_sampling="none", dg_dense_grid=True, dg_outputs="reduced", fps_sample_decay=False, dropout=True), ()),
    "lhp_depth_term": (dict(lhp=True, lhp_weight=0.3), ()),
    "lhp_cached": (dict(lhp=True, lhp_weight=0.3, dg_feature_cache="float32"), ("feats",)),
    "pair_cached": (dict(dg_feature_cache="float32"), ("feats",)),
    "depth_none": (dict(arch="dino_depth", guidance="none"), ()),
    "depth_sum_rec": (dict(DEPTH, rec_weight=0.5, dg_rec_feats_grad=True), ()),
    "depth_only_intra": (dict(DEPTH, use_depth_only_intra=True, depth_feat_correlation_loss=False, depth_sampling="none", dg_outputs="reduced",
                              fps_sample_decay=False), ()),
    "pair_rec": (dict(rec_weight=0.5), ()),
    "aug_batch_keys": (dict(aug_alignment_weight=0.5), ("aug",)),
    "aug_gpu_unit": (dict(aug_alignment_weight=0.5, dg_gpu_augment="unit"), ()),
    "crf": (dict(crf_weight=0.5), ()),
    "hist_every_step": (dict(hist_freq=1), ()),
    "reset_probe": (dict(reset_probe_steps=1), ()),
    "fused_adam": (dict(dg_fused_adam=True), ()),
    "fused_adam_bucket": (dict(dg_fused_adam=True), ("bucket",)),
    "no_correspondence": (dict(correspondence_weight=0.0), ()),
}


def make_batch(dev, seg, extras):
    from depthg_amd.aug_loss import crop_flip_coords
    g = torch.Generator().manual_seed(1)
    batch = {"img": torch.randn(B, 3, HW, HW, generator=g), "img_pos": torch.randn(B, 3, HW, HW, generator=g),
             "label": torch.randint(0, N_CLASSES, (B, HW, HW), generator=g),
             "depth": torch.randint(1, 256, (B, 1, HW, HW), generator=g).float(),
             "depth_pos": torch.randint(1, 256, (B, 1, HW, HW), generator=g).float()}
    if "aug" in extras:
        batch["img_aug"] = torch.randn(B, 3, HW, HW, generator=g)
        batch["coord_aug"] = crop_flip_coords(B, HW, HW, [(4.0, 2.0, 50.0, 56.0), (0.0, 6.0, 60.5, 52.0)], [False, True])
    batch = {k: v.to(dev) for k, v in batch.items()}
    if "feats" in extras:
        with torch.no_grad():
            batch["image_feat"], batch["image_feat_pos"] = seg.net._backbone(batch["img"])[0], seg.net._backbone(batch["img_pos"])[0]
    return batch


def run(name, dev):
    """-> {quantity: [tensors]} of three seeded steps of configuration `name`."""
    from depthg_amd.parallel import GradBucket
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    over, extras = MATRIX[name]
    torch.manual_seed(3)
    seg = UnsupervisedSegmenter(N_CLASSES, default_segmenter_cfg(**{**BASE, **over})).to(dev).train()
    batch = make_batch(dev, seg, extras)
    grad_sync = None
    if "bucket" in extras:
        bucket = GradBucket.for_parameters(seg.all_reduced_parameters())
        grad_sync = lambda: [bucket.pack(), bucket.allreduce_mean_(), bucket][-1]
    torch.manual_seed(7)
    losses, logs = [], []
    for step in range(3):
        loss, log = seg.training_step(batch, step, grad_sync=grad_sync)
        losses.append(loss.detach().clone())
        logs += [log[k].detach().clone() for k in sorted(log)]
    torch.cuda.synchronize()
    assert seg.global_step == 3 and all(bool(torch.isfinite(v)) for v in losses), (name, losses)
    return {"loss": losses, "logs": logs, "params": [p.detach() for p in seg.parameters()],
            "rng": [torch.get_rng_state(), torch.cuda.get_rng_state(dev)]}


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def compare(path_a, path_b):
    a, b = torch.load(path_a), torch.load(path_b)
    for name in a:
        worst = {q: max((float((u.double() - v.double()).abs().max()) for u, v in zip(a[name][q], b[name][q]) if u.numel()), default=0.0)
                 for q in a[name]}
        print(json.dumps({"config": name, "max_abs_difference": worst}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=os.path.join("profiles", "step_stages.jsonl"))
    ap.add_argument("--values", default=None)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--deterministic", action="store_true")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    sys.path.insert(0, os.path.abspath(args.tree))
    dev = torch.device("cuda:0")
    torch.backends.cudnn.deterministic = args.deterministic
    values = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for name in args.only or MATRIX:
            values[name] = {q: [t.cpu() for t in ts] for q, ts in run(name, dev).items()}
            line = json.dumps({"config": name, **{q: digest(ts) for q, ts in values[name].items()}})
            print(line, flush=True)
            out.write(line + "\n")
    if args.values:
        torch.save(values, args.values)


if __name__ == "__main__":
    main()
