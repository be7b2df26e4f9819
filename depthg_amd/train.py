"""Train a segmenter from a dataset folder: the loop of src/train_segmentation.py:551-714 without Lightning, Hydra, TensorBoard or wandb.

    python -m depthg_amd.train --data-dir D --out O [--dataset directory] [--precompute-knns] [--feature-cache float32] [--val-feature-cache float32] [--sample-cache] [--device cuda:0] [key=value ...]

builds the train pipeline (data.CroppedFolder, or data.DirectoryFolder with --dataset directory, under data.ContrastiveBatches: the
loader transform of a batch and its kNN positives is one fused HIP launch) from the cfg keys dataset_name, crop_type, crop_ratio, res,
loader_crop_type, num_neighbors, use_depth, depth_type, batch_size and max_steps, the val pipeline at eval_res 320 (224 for model_type
"mae") with a centre crop (none for dataset_name "voc"), an UnsupervisedSegmenter, and runs `fit`.  Keys come from
segmenter.default_segmenter_cfg and TRAIN_DEFAULTS, overridden by `key=value` arguments (values are read as Python literals where
they parse, else as strings; `~` and `null` are None).  --precompute-knns writes a missing nearest-neighbour table first
(data.precompute_knns).  --feature-cache {float32,float16,bfloat16} (cfg.dg_feature_cache) runs the frozen backbone over the train split
once behind that, keeps its features in a feature_cache.FeatureCache - saved as <data-dir>/feature_cache_<meta>.pt and loaded from there when
the file exists and matches - and trains from them: the step skips the backbone (loader_crop_type "center" or None, arch "dino"; validation
is untouched).  --val-feature-cache {float32,float16,bfloat16} (cfg.dg_val_feature_cache) does the same for the val split, behind the
train cache: the backbone runs over the val images once, at eval_res and the val crop (val_feature_cache; the file's metadata name the
split, so a train file is never taken for it), every val batch carries `image_feat` from one gather launch, and validation_step starts
behind the backbone - the eval-mode head, then the fused probe-and-score launches, as ever; with a float32 cache its predictions and
metrics are those of the uncached validation.  --feature-cache alone leaves validation as it was.  --sample-cache keeps the loader's output bytes of the train and the val split on the device (sample_cache.SampleCache,
saved as <data-dir>/sample_cache_<meta>.pt and loaded from there when the file matches): every batch is then one gather launch over them
and an epoch opens no image file; without the flag nothing changes.  --graph-step (cfg.dg_graph_step; with both caches) draws every batch
and its positives on the device (epoch.DeviceEpoch) and replays the step from a hipGraph (graph_step.GraphedTrainStep): the short last
batch of an epoch is dropped and the positives come from the epoch's own random stream.  The reference reads its val set from the uncropped dataset classes; here both splits come from the same
folder layout (cfg.val_crop_type names the val folder's crop, default: cfg.crop_type).

`fit(model, train_batches, val_batches, cfg, out_dir)`:
    training_step per batch, epoch after epoch, until cfg.max_steps;
    every cfg.val_freq batches of an epoch: validation_step over val_batches, then on_validation_epoch_end.  A val_freq above a quarter
        of an epoch is dropped, as in the reference (:690-691): validation then runs at the end of every epoch.  The fit's last step is
        always followed by a validation (unless one just ran), so the checkpoints it leaves carry metrics of their own weights;
    <out_dir>/last.pt after every validation and at the end, <out_dir>/best.pt whenever `test/cluster/mIoU` (`test/cluster/Accuracy`
        for dataset_name "potsdam") exceeds its best so far - both through demo.save_checkpoint;
    <out_dir>/log.jsonl: one JSON line {"step": n, ...the step's logs} every cfg.scalar_log_freq steps and one {"step": n, "val": {...}}
        per validation.
"""
import argparse
import ast
import json
import os
import sys

import torch

from .segmenter import UnsupervisedSegmenter, default_segmenter_cfg

# the loop's and the pipelines' keys, with the values of src/configs/local_config.yml
TRAIN_DEFAULTS = dict(dataset_name="cocostuff27", crop_type="five", crop_ratio=.5, res=224, loader_crop_type="center", num_neighbors=7,
                      depth_type="zoedepth", batch_size=32, max_steps=7000, val_freq=100, scalar_log_freq=10, num_workers=8,
                      dir_dataset_name=None, dir_dataset_n_classes=5, val_crop_type=None)


def monitor_key(cfg):
    return "test/cluster/Accuracy" if getattr(cfg, "dataset_name", None) == "potsdam" else "test/cluster/mIoU"      # :693-696


def validation_interval(cfg, batches_per_epoch):
    """cfg.val_freq in batches, or None (validate at the end of every epoch) when there is none or it exceeds a quarter of an epoch."""
    val_freq = getattr(cfg, "val_freq", None)
    if val_freq is None or int(val_freq) < 1 or int(val_freq) > batches_per_epoch // 4:                              # :690-691
        return None
    return int(val_freq)


def _plain(v):
    if isinstance(v, torch.Tensor):
        return float(v) if v.numel() == 1 else v.detach().cpu().tolist()
    return v.item() if hasattr(v, "item") else v


def fit(model, train_batches, val_batches, cfg, out_dir, save_checkpoint=None, graph_step=None):
    """See the module docstring.  `save_checkpoint(model, path)`: demo.save_checkpoint unless given.  Returns {"steps", "validations",
    "val_steps" (the step counts validations ran behind), "best", "best_step", "losses"}.
    `graph_step`: a graph_step.GraphedTrainStep (cfg.dg_graph_step) - the same loop over its step(), an epoch being the
    steps_per_epoch batches of its DeviceEpoch behind a begin_epoch(); `train_batches` is then not read.  The losses stay on the device
    until the loop ends (no synchronisation per step)."""
    if save_checkpoint is None:
        from .demo import save_checkpoint
    os.makedirs(out_dir, exist_ok=True)
    max_steps = int(cfg.max_steps)
    per_epoch = len(train_batches) if graph_step is None else graph_step.epoch.steps_per_epoch
    if per_epoch < 1:
        raise ValueError("depthg_amd.train: the train pipeline has no batch")
    interval = validation_interval(cfg, per_epoch)
    log_freq = max(int(getattr(cfg, "scalar_log_freq", 10)), 1)
    monitor = monitor_key(cfg)
    log_path = os.path.join(out_dir, "log.jsonl")
    state = {"steps": 0, "validations": 0, "val_steps": [], "best": None, "best_step": None, "losses": []}

    def write(line):
        with open(log_path, "a") as f:
            f.write(json.dumps(line) + "\n")

    def validate():
        if val_batches is None:
            return
        for i, batch in enumerate(val_batches):
            model.validation_step(batch, i)
        metrics = {k: _plain(v) for k, v in model.on_validation_epoch_end().items()}
        state["validations"] += 1
        state["val_steps"].append(state["steps"])
        write({"step": state["steps"], "val": metrics})
        save_checkpoint(model, os.path.join(out_dir, "last.pt"))
        score = metrics.get(monitor)
        if score is not None and (state["best"] is None or score > state["best"]):
            state["best"], state["best_step"] = score, state["steps"]
            save_checkpoint(model, os.path.join(out_dir, "best.pt"))

    def epoch_steps():
        """(batch_idx, (loss, logs)) of one epoch, each step run when it is asked for."""
        if graph_step is None:
            for batch_idx, batch in enumerate(train_batches):
                yield batch_idx, model.training_step(batch, batch_idx)
        else:
            graph_step.epoch.begin_epoch()
            for batch_idx in range(per_epoch):
                loss, logs = graph_step.step()
                yield batch_idx, (loss.clone(), logs)            # (a replay's tensors are the recording's own: the next step overwrites them)

    while state["steps"] < max_steps:
        for batch_idx, (loss, logs) in epoch_steps():
            state["steps"] += 1
            state["losses"].append(float(loss) if graph_step is None else loss)
            if state["steps"] % log_freq == 0:
                write({"step": state["steps"], **{k: _plain(v) for k, v in logs.items()}})
            last_of_epoch = batch_idx + 1 == per_epoch
            if (interval is not None and (batch_idx + 1) % interval == 0) or (interval is None and last_of_epoch):
                validate()
            if state["steps"] >= max_steps:
                break
    if not state["val_steps"] or state["val_steps"][-1] != state["steps"]:
        validate()
    save_checkpoint(model, os.path.join(out_dir, "last.pt"))
    if graph_step is not None and state["losses"]:
        state["losses"] = torch.stack(state["losses"]).tolist()
    return state


# --------------------------------------------------------------------------------------------------------------- command line
def parse_overrides(pairs):
    out = {}
    for pair in pairs:
        key, sep, text = pair.partition("=")
        if not sep or not key:
            raise ValueError("Unexpected arg style {}".format(pair))                                                 # src/utils.py:160
        if text in ("~", "null", "None"):
            out[key] = None
            continue
        try:
            out[key] = ast.literal_eval(text)
        except (ValueError, SyntaxError):
            out[key] = text
    return out


def build_cfg(overrides):
    cfg = default_segmenter_cfg(**{**TRAIN_DEFAULTS, **overrides})
    return cfg


def build_dataset(cfg, data_dir, image_set, return_depth):
    from . import data
    if cfg.dataset_name == "directory":
        return data.DirectoryFolder(data_dir, image_set, name=cfg.dir_dataset_name or "directory", n_classes=cfg.dir_dataset_n_classes,
                                    crop_type=cfg.crop_type if image_set == "train" else None)
    crop = cfg.crop_type if image_set == "train" or cfg.val_crop_type is None else cfg.val_crop_type
    return data.CroppedFolder(data_dir, cfg.dataset_name, crop, cfg.crop_ratio, image_set, return_depth=return_depth, depth_type=cfg.depth_type)


def train_feature_cache(cfg, data_dir, device, train_set, net, dtype, sample_cache=None):
    """The train split's feature_cache.FeatureCache of storage type `dtype`: loaded from <data_dir>/feature_cache_<meta>.pt when that file
    exists and its metadata match, else built with the featurizer `net` (data.build_feature_cache) and saved there.  `sample_cache`: an
    empty sample cache of the split that the building pass fills from the samples it decodes (left empty when the file is loaded)."""
    from . import data
    from .feature_cache import FeatureCache
    meta = data.feature_cache_meta(cfg, train_set, cfg.res, cfg.loader_crop_type)
    path = data.feature_cache_path(data_dir, meta, "train", dtype)
    if os.path.exists(path):
        try:
            cache = FeatureCache.load(path, device, expect_meta=meta)
            if bool(cache.filled.all()):
                print(f"depthg_amd.train: feature cache loaded from {path} ({cache.nbytes} bytes)")
                return cache
        except ValueError as e:
            print(f"depthg_amd.train: {path} does not match ({e}); rebuilding")
    cache = data.build_feature_cache(net, train_set, cfg, cfg.res, cfg.loader_crop_type, dtype=dtype, device=device,
                                     batch_size=min(128 if cfg.model_type == "vit_small" else 64, max(len(train_set), 1)),
                                     num_workers=cfg.num_workers, sample_cache=sample_cache)
    cache.save(path)
    print(f"depthg_amd.train: feature cache built and saved to {path} ({cache.nbytes} bytes)")
    return cache


def val_view(cfg):
    """(eval_res, val_crop): the val pipeline's loader transform - 320 (224 for model_type "mae"), a centre crop (none for "voc")."""
    return (224 if cfg.model_type == "mae" else 320), (None if cfg.dataset_name == "voc" else "center")          # :597-600, :632-635


def val_feature_cache(cfg, data_dir, device, val_set, net, dtype, sample_cache=None):
    """The VAL split's feature_cache.FeatureCache of storage type `dtype`, at the val pipeline's view (val_view: eval_res and the val
    crop): loaded from <data_dir>/feature_cache_<meta>.pt when that file exists and its metadata match - the split ("val"), the
    resolution, the crop and the image count among them, so the train split's file is never taken for it - else built with the
    featurizer `net` (data.build_feature_cache) and saved there.  `sample_cache`: an empty sample cache of the val split that the
    building pass fills from the samples it decodes (left empty when the file is loaded).  The table takes n * C * h * w * itemsize
    bytes on the device; one that does not fit fails with the bytes named (row_cache.RowCache)."""
    from . import data
    from .feature_cache import FeatureCache
    eval_res, val_crop = val_view(cfg)
    meta = data.feature_cache_meta(cfg, val_set, eval_res, val_crop, image_set="val")
    path = data.feature_cache_path(data_dir, meta, "val", dtype)
    if os.path.exists(path):
        try:
            cache = FeatureCache.load(path, device, expect_meta=meta)
            if bool(cache.filled.all()):
                print(f"depthg_amd.train: val feature cache loaded from {path} ({cache.nbytes} bytes)")
                return cache
        except ValueError as e:
            print(f"depthg_amd.train: {path} does not match ({e}); rebuilding")
    cache = data.build_feature_cache(net, val_set, cfg, eval_res, val_crop, dtype=dtype, device=device,
                                     batch_size=min(int(cfg.batch_size), max(len(val_set), 1)), num_workers=cfg.num_workers,
                                     sample_cache=sample_cache, image_set="val")
    cache.save(path)
    print(f"depthg_amd.train: val feature cache built and saved to {path} ({cache.nbytes} bytes)")
    return cache


def load_sample_cache(data_dir, device, dataset, image_set, res, crop_type, want_depth):
    """(cache, path): the split's sample_cache.SampleCache from <data_dir>/sample_cache_<meta>.pt when that file exists, its metadata
    match and every row is there - else an EMPTY cache for the caller to fill (finish_sample_cache) and save there."""
    from . import data
    from .sample_cache import SampleCache
    meta = data.sample_cache_meta(dataset, image_set, res, crop_type, want_depth)
    path = data.sample_cache_path(data_dir, meta)
    if os.path.exists(path):
        try:
            cache = SampleCache.load(path, device, expect_meta=meta)
            if bool(cache.filled.all()):
                print(f"depthg_amd.train: sample cache loaded from {path} ({cache.nbytes} bytes)")
                return cache, path
        except ValueError as e:
            print(f"depthg_amd.train: {path} does not match ({e}); rebuilding")
    return data.new_sample_cache(dataset, image_set, res, crop_type, want_depth, device), path


def finish_sample_cache(cfg, cache, path, dataset, res, crop_type):
    """Fill the rows of `cache` that no earlier pass has put (all of them, unless the feature cache's building pass did) and save it."""
    from . import data
    if bool(cache.filled.all()) and os.path.exists(path):
        return cache
    data.fill_sample_cache(cache, dataset, res, crop_type, num_workers=cfg.num_workers)
    cache.save(path)
    print(f"depthg_amd.train: sample cache built and saved to {path} ({cache.nbytes} bytes)")
    return cache


def build_pipelines(cfg, data_dir, device, precompute=False, net=None, feature_cache=None, sample_cache=False, val_cache=None):
    """(train_batches, val_batches, n_classes) of cfg (:614-658).  `precompute`: write the train table first when it is missing, with `net`.
    `feature_cache`: None, or the storage type of the train split's feature cache (train_feature_cache; `net` supplies the featurizer).
    `sample_cache`: keep both splits' loader outputs on the device (--sample-cache); with a feature cache to build as well, the train
    split is decoded once for both.  `val_cache`: None, or the storage type of the val split's feature cache (val_feature_cache, built
    or loaded behind the train one): the val batches then carry `image_feat`."""
    from . import data, knn
    train_set = build_dataset(cfg, data_dir, "train", bool(cfg.use_depth))
    if train_set.n_classes is None:
        raise ValueError(f"Unknown dataset: {cfg.dataset_name}")                                                    # src/data.py:1039
    path = knn.nns_path(data_dir, cfg.model_type, train_set.nns_name, "train", train_set.crop_type, cfg.res)
    if precompute and not os.path.exists(path):
        data.precompute_knns(net(train_set.n_classes), train_set, cfg, cfg.res, "train", train_set.crop_type, num_workers=cfg.num_workers,
                             device=device, batch_size=min(128 if cfg.model_type == "vit_small" else 64, max(len(train_set), 1)))
    cache = samples = val_samples = None
    if sample_cache:
        samples, samples_path = load_sample_cache(data_dir, device, train_set, "train", cfg.res, cfg.loader_crop_type, bool(cfg.use_depth))
    if feature_cache is not None:
        cache = train_feature_cache(cfg, data_dir, device, train_set, net(train_set.n_classes), feature_cache,
                                    sample_cache=samples if samples is not None and not samples.filled.any() else None)
    if sample_cache:
        finish_sample_cache(cfg, samples, samples_path, train_set, cfg.res, cfg.loader_crop_type)
    gen = torch.Generator().manual_seed(0)                                                                           # seed_everything(0), :590
    train_batches = data.ContrastiveBatches(train_set, cfg, "train", cfg.res, cfg.loader_crop_type, cfg.batch_size, shuffle=True, generator=gen,
                                            num_workers=cfg.num_workers, pos=True, return_depth=bool(cfg.use_depth), device=device,
                                            feature_cache=cache, sample_cache=samples)
    eval_res, val_crop = val_view(cfg)
    val_set = build_dataset(cfg, data_dir, "val", False)
    val_feats = None
    if sample_cache:
        val_samples, val_path = load_sample_cache(data_dir, device, val_set, "val", eval_res, val_crop, False)
    if val_cache is not None:
        val_feats = val_feature_cache(cfg, data_dir, device, val_set, net(train_set.n_classes), val_cache,
                                      sample_cache=val_samples if val_samples is not None and not val_samples.filled.any() else None)
    if sample_cache:
        finish_sample_cache(cfg, val_samples, val_path, val_set, eval_res, val_crop)
    val_batches = data.ContrastiveBatches(val_set, cfg, "val", eval_res, val_crop, cfg.batch_size, shuffle=False, num_workers=cfg.num_workers,
                                          pos=False, return_depth=False, device=device, feature_cache=val_feats, sample_cache=val_samples)
    return train_batches, val_batches, train_set.n_classes


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m depthg_amd.train", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--dataset", default=None, help="`directory`: imgs/{split} and labels/{split} under --data-dir (sets dataset_name)")
    ap.add_argument("--precompute-knns", action="store_true", help="write the nearest-neighbour table first when it is missing")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--feature-cache", choices=("float32", "float16", "bfloat16"), default=None,
                    help="keep the frozen backbone's features of the train split in this type and train from them (sets dg_feature_cache); "
                         "built once, saved as feature_cache_<meta>.pt under --data-dir and loaded from there afterwards")
    ap.add_argument("--val-feature-cache", choices=("float32", "float16", "bfloat16"), default=None,
                    help="keep the frozen backbone's features of the VAL split (at eval_res, the val crop) in this type and validate from "
                         "them (sets dg_val_feature_cache); built once behind the train cache, saved as feature_cache_<meta>.pt under "
                         "--data-dir and loaded from there afterwards")
    ap.add_argument("--sample-cache", action="store_true",
                    help="keep the loader's output bytes of the train and the val split on the device and form every batch from them in one "
                         "launch; built once, saved as sample_cache_<meta>.pt under --data-dir and loaded from there afterwards "
                         "(loader_crop_type 'center' or None)")
    ap.add_argument("--graph-step", action="store_true",
                    help="record the cached training step in a hipGraph and replay it, the batches drawn on the device (sets dg_graph_step, and "
                         "dg_graph_safe and dg_fused_adam unless given); needs --feature-cache and --sample-cache; the short last batch of an "
                         "epoch is dropped")
    ap.add_argument("--fused-probes", action="store_true",
                    help="train the linear and the cluster probe through one fused HIP operation per step (sets dg_fused_probes)")
    ap.add_argument("overrides", nargs="*", help="cfg keys as key=value")
    args = ap.parse_args(argv)
    overrides = parse_overrides(args.overrides)
    if args.dataset is not None:
        overrides["dataset_name"] = args.dataset
    if args.feature_cache is not None:
        overrides["dg_feature_cache"] = args.feature_cache
    if args.val_feature_cache is not None:
        overrides["dg_val_feature_cache"] = args.val_feature_cache
    if args.fused_probes:
        overrides["dg_fused_probes"] = True
    if args.graph_step:
        if args.feature_cache is None or not args.sample_cache:
            ap.error("--graph-step replays the CACHED step: give --feature-cache {float32,float16,bfloat16} and --sample-cache as well")
        overrides["dg_graph_step"] = True
        overrides.setdefault("dg_graph_safe", True)              # (given as False they are refused by GraphedTrainStep, with the way out)
        overrides.setdefault("dg_fused_adam", True)
    cfg = build_cfg(overrides)
    if getattr(cfg, "dg_feature_cache", None) and getattr(cfg, "arch", "dino") == "dino_depth":
        raise ValueError("depthg_amd.train: --feature-cache serves cfg.arch = 'dino'; the depth-guided featurizer (arch 'dino_depth') is out of "
                         "scope for the feature cache")
    if not torch.cuda.is_available():
        sys.exit("depthg_amd.train: no GPU (training_step has no CPU route)")
    device = torch.device(args.device)
    torch.manual_seed(0)                                                                                             # :590
    holder = {}

    def model_for(n_classes):
        if "model" not in holder:
            holder["model"] = UnsupervisedSegmenter(n_classes, cfg).to(device)
        return holder["model"]

    def knn_net(n_classes):
        model = model_for(n_classes)
        if model.depth_arch:
            raise ValueError("depthg_amd.train: --precompute-knns pools the image featurizer's output; with cfg.arch = 'dino_depth' write the "
                             "table under arch='dino' first")
        return model.net

    train_batches, val_batches, n_classes = build_pipelines(cfg, args.data_dir, device, args.precompute_knns, knn_net,
                                                            getattr(cfg, "dg_feature_cache", None), args.sample_cache,
                                                            getattr(cfg, "dg_val_feature_cache", None))
    model = model_for(n_classes)
    model.train()
    graph_step = None
    if getattr(cfg, "dg_graph_step", False):
        from .epoch import DeviceEpoch
        from .graph_step import GraphedTrainStep
        epoch = DeviceEpoch(train_batches.nns, cfg.batch_size, train_batches.num_neighbors, device, shuffle=True, generator=train_batches.generator)
        graph_step = GraphedTrainStep(model, epoch, train_batches.sample_cache, train_batches.feature_cache,
                                      label_dims=train_batches.dataset.label_dims)
    state = fit(model, train_batches, val_batches, cfg, args.out, graph_step=graph_step)
    if graph_step is not None:
        print(f"depthg_amd.train: {graph_step.captures} recording(s) of the step")
    print(f"depthg_amd.train: {state['steps']} step(s), {state['validations']} validation(s), best {monitor_key(cfg)} = {state['best']} "
          f"at step {state['best_step']} -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
