"""The validation feature cache on the GPU (cfg.dg_val_feature_cache): validation_step and evaluate_batch from cached features against
the same calls through the backbone - the stand-in featurizer and a two-block ViT, 32 x 32 and 48 x 32 images (grids of 4 x 4 and
6 x 4: below one tile, and not square), 5 images at batch size 2 (a short last batch), deterministic torch algorithms (as
tests/test_gpu_feature_cache.py).  Every float32 case runs the uncached route twice first (A, A'): where the pair agrees the cached
run C must equal it in everything; where it does not, that is reported and C is held to equality with A or with A' on the integer
results (prediction maps, confusion counts).  The 16-bit caches are held, bit for bit, to predict_and_score on
forward_features(image_feat.to(T).float()).  Then the single-list gather against the CPU route, `fit` with and without the cache,
with and without the graphed step, and the train command."""
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

import data_folders as DF
from conftest import ROOT
from epoch_draw_reference import case
from feature_cache_cases import exact_widen, feature_rows
from sample_cache_cases import CROPPED, MemorySet, make_samples

pytestmark = pytest.mark.gpu

N_VAL, N_CLASSES, BATCH = 5, 5, 2
SIZES_HW = {"32x32": (32, 32), "48x32": (48, 32)}
BATCHES = [[0, 1], [2, 3], [4]]
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def deterministic(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


def _cfg(kind, **over):
    from depthg_amd.segmenter import default_segmenter_cfg
    if kind == "dino":          # a two-block ViT (head dimension 64)
        base = dict(model_type="vit_small", dino_patch_size=8, dg_dino_backbone=True, feature_samples=5,
                    dg_dino_vit_kwargs=dict(img_size=[32], embed_dim=128, depth=2, num_heads=2))
    else:                       # the stand-in backbone: 384 channels
        base = dict(dim=70, feature_samples=5)
    return default_segmenter_cfg(**{**base, **over})


def _segmenter(kind, dev, **over):
    from depthg_amd.segmenter import UnsupervisedSegmenter
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)            # (the ViT keeps its seeded random weights)
        seg = UnsupervisedSegmenter(N_CLASSES, _cfg(kind, **over)).to(dev)
    seg.train()
    return seg


_SPLITS = {}


def _split(size, dev):
    """(img (5,3,H,W), label (5,H,W)) of one image size, drawn once and never changed."""
    if size not in _SPLITS:
        H, W = SIZES_HW[size]
        g = torch.Generator().manual_seed(11 + H)
        _SPLITS[size] = (torch.randn(N_VAL, 3, H, W, generator=g).to(dev), torch.randint(-1, N_CLASSES, (N_VAL, H, W), generator=g).to(dev))
    return _SPLITS[size]


def _caches(seg, img, dtype, mirrored=False):
    """The split's FeatureCache (and the mirrored images' one), filled as data.build_feature_cache fills them: the backbone in eval mode
    under no_grad, one put per batch."""
    from depthg_amd import FeatureCache
    out = []
    seg.net.model.eval()
    with torch.no_grad():
        for flip in ((False, True) if mirrored else (False,)):
            cache = None
            for inds in BATCHES:
                x = img[inds].flip(dims=[3]) if flip else img[inds]
                f = seg.net._backbone(x)[0]
                if cache is None:
                    cache = FeatureCache(N_VAL, *f.shape[1:], dtype=dtype, device=img.device)
                cache.put(inds, f)
            out.append(cache)
    return out


def _batches(img, label, cache=None, mirrored=None):
    for inds in BATCHES:
        batch = {"ind": torch.tensor(inds), "img": img[inds], "label": label[inds]}
        if cache is not None:
            batch["image_feat"] = cache.gather(inds)
        if mirrored is not None:
            batch["image_feat_flip"] = mirrored.gather(inds)
        yield batch


def _no_backbone(seg, monkeypatch):
    monkeypatch.setattr(seg.net, "_backbone", lambda *a, **k: pytest.fail("the cached route ran the backbone"))


def _validation(seg, batches):
    """One validation pass -> {"ints": the integer results, "rest": everything else}."""
    outs = [seg.validation_step(batch, i) for i, batch in enumerate(batches)]
    assert seg.net.training
    stats = [seg.linear_metrics.stats.cpu().clone(), seg.cluster_metrics.stats.cpu().clone()]
    metrics = seg.on_validation_epoch_end()
    torch.cuda.synchronize()
    return {"ints": [o[k] for o in outs for k in ("linear_preds", "cluster_preds", "label")] + stats,
            "rest": [o["img"] for o in outs] + [torch.tensor([metrics[k] for k in sorted(metrics)], dtype=torch.float64)],
            "keys": sorted(metrics)}


def _evaluation(seg, batches, run_crf):
    preds = [seg.evaluate_batch(batch, flip=True, run_crf=run_crf) for batch in batches]
    stats = [seg.test_linear_metrics.stats.cpu().clone(), seg.test_cluster_metrics.stats.cpu().clone()]
    metrics = {**seg.test_linear_metrics.compute(), **seg.test_cluster_metrics.compute()}
    seg.test_linear_metrics.reset()
    seg.test_cluster_metrics.reset()
    torch.cuda.synchronize()
    return {"ints": [p.cpu() for pair in preds for p in pair] + stats,
            "rest": [torch.tensor([metrics[k] for k in sorted(metrics)], dtype=torch.float64)], "keys": sorted(metrics)}


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and
                                    torch.equal(x.reshape(-1).contiguous().view(torch.uint8), y.reshape(-1).contiguous().view(torch.uint8))
                                    for x, y in zip(a, b))


def _hold(what, A, A2, C):
    """The rule of the module docstring."""
    assert A["keys"] == A2["keys"] == C["keys"] and len(A["ints"]) == len(C["ints"])
    assert int(A["ints"][-1].sum()) > 0 and int(A["ints"][-2].sum()) > 0, "nothing was counted"
    if _same(A["ints"], A2["ints"]) and _same(A["rest"], A2["rest"]):
        assert _same(A["ints"], C["ints"]), f"{what}: the uncached pair agrees, the cached run's predictions or counts differ"
        assert _same(A["rest"], C["rest"]), f"{what}: the uncached pair agrees, the cached run's metrics or images differ"
    else:
        differ = [i for i, (x, y) in enumerate(zip(A["ints"], A2["ints"])) if not torch.equal(x, y)]
        print(f"{what}: two uncached runs do NOT agree on this machine (integer results {differ} differ)")
        assert _same(A["ints"], C["ints"]) or _same(A2["ints"], C["ints"]), f"{what}: the cached run equals neither uncached run"


CASES = [(kind, size) for kind in ("standin", "dino") for size in SIZES_HW]
IDS = [f"{k}-{s}" for k, s in CASES]


@pytest.mark.parametrize("kind,size", CASES, ids=IDS)
def test_float32_cache_validation_equals_the_uncached(kind, size, dev, monkeypatch):
    img, label = _split(size, dev)
    seg = _segmenter(kind, dev)
    A = _validation(seg, _batches(img, label))
    A2 = _validation(seg, _batches(img, label))
    cache, = _caches(seg, img, torch.float32)
    h, w = SIZES_HW[size][0] // 8, SIZES_HW[size][1] // 8
    assert cache.shape == (seg.net.n_feats, h, w)
    seg.cfg.dg_val_feature_cache = "float32"
    _no_backbone(seg, monkeypatch)
    C = _validation(seg, _batches(img, label, cache))
    assert [t.shape[0] for t in C["ints"][0:9:3]] == [2, 2, 1]
    _hold(f"validation {kind} {size}", A, A2, C)


@pytest.mark.parametrize("run_crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("kind,size", CASES, ids=IDS)
def test_float32_caches_evaluate_batch_with_flip(kind, size, run_crf, dev, monkeypatch):
    img, label = _split(size, dev)
    seg = _segmenter(kind, dev)
    A = _evaluation(seg, _batches(img, label), run_crf)
    A2 = _evaluation(seg, _batches(img, label), run_crf)
    cache, mirrored = _caches(seg, img, torch.float32, mirrored=True)
    seg.cfg.dg_val_feature_cache = "float32"
    _no_backbone(seg, monkeypatch)
    C = _evaluation(seg, _batches(img, label, cache, mirrored), run_crf)
    _hold(f"evaluate_batch {kind} {size} run_crf={run_crf}", A, A2, C)
    # a mirrored feature map in place of the mirrored images' features is refused where it can be told: by its absence
    with pytest.raises(ValueError, match="mirrored=True"):
        seg.evaluate_batch(next(_batches(img, label, cache)), flip=True)


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
@pytest.mark.parametrize("kind,size", CASES, ids=IDS)
def test_16_bit_caches_equal_the_head_on_the_rounded_features(kind, size, name, dev, monkeypatch):
    from depthg_amd.evaluation import predict_and_score
    from depthg_amd.metrics import UnsupervisedMetrics
    T = DTYPES[name]
    img, label = _split(size, dev)
    seg = _segmenter(kind, dev)
    k = seg.cfg.n_images
    # the statement: the eval-mode head on the features rounded to T and widened, then the uncached probe-and-score
    lin, clu = UnsupervisedMetrics("test/linear/", N_CLASSES, 0, False), UnsupervisedMetrics("test/cluster/", N_CLASSES, 0, True)
    want = []
    seg.net.eval()
    with torch.no_grad():
        for inds in BATCHES:
            f = seg.net._backbone(img[inds])[0]
            code = seg.net.forward_features(f.to(T).float())[1]
            want += [p.cpu() for p in predict_and_score(code, label[inds], seg.linear_probe, seg.cluster_probe, lin, clu, n_store=k)]
    seg.net.train()
    torch.cuda.synchronize()
    cache, = _caches(seg, img, T)
    assert cache.dtype == T and cache.nbytes == N_VAL * seg.net.n_feats * (SIZES_HW[size][0] // 8) * (SIZES_HW[size][1] // 8) * 2
    seg.cfg.dg_val_feature_cache = name
    _no_backbone(seg, monkeypatch)
    outs = [seg.validation_step(batch, i) for i, batch in enumerate(_batches(img, label, cache))]
    got = [o[key] for o in outs for key in ("linear_preds", "cluster_preds")]
    assert _same(want, got)
    assert torch.equal(seg.linear_metrics.stats.cpu(), lin.stats.cpu()) and torch.equal(seg.cluster_metrics.stats.cpu(), clu.stats.cpu())
    assert int(lin.stats.sum()) > 0
    res, ref = seg.on_validation_epoch_end(), {**lin.compute(), **clu.compute()}
    assert len(ref) == 4 and all(res[key] == value for key, value in ref.items())


# ---------------------------------------------------------------------------------------------------------------- the gather
# (C, h, w), N, rows put, the single list, a second list for the paired call:
#   L = 105: odd - 16-bit rows start off a 16-byte boundary; L = 128: whole vectors, an empty tail; n = 1: a one-row batch;
#   L = 6144 = 384 x 4 x 4: the stand-in's row at 32 x 32
GATHERS = [((3, 5, 7), 7, [6, 0, 3, 2, 5], [0, 6, 3], [5, 2, 0]),
           ((8, 4, 4), 4, [3, 1, 0], [1, 0, 3, 1], [0, 0, 1, 3]),
           ((3, 5, 7), 4, [2, 3], [3], [2]),
           ((384, 4, 4), 5, [0, 1, 2, 3, 4], [4], [0])]


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("shape,N,put,ind,ind_pos", GATHERS, ids=["L105", "L128", "L105-one-row", "L6144-one-row"])
def test_single_list_gather_matches_the_cpu_route(shape, N, put, ind, ind_pos, name, dev, monkeypatch):
    from depthg_amd import FeatureCache, ops
    dtype = DTYPES[name]
    L = shape[0] * shape[1] * shape[2]
    x = feature_rows(len(put), *shape, seed=len(put))
    ref, gpu = FeatureCache(N, *shape, dtype=dtype, device="cpu"), FeatureCache(N, *shape, dtype=dtype, device=dev)
    ref.put(put, x)
    gpu.put(put, x.to(dev))

    def rows_of(idx):          # the CPU route's stored rows widened exactly (the NaN payloads: feature_cache_cases.exact_widen)
        return exact_widen(ref.data.index_select(0, torch.tensor(idx))).reshape((len(idx),) + shape)

    def bits(t):
        return t.contiguous().cpu().view(torch.int32)

    want, want_pos = rows_of(ind), rows_of(ind_pos)
    # every element of a poisoned output is written (0xFF bytes: what DG_POISON=1 fills the buffers with), by one call
    monkeypatch.setattr(ops, "POISON", True)
    calls, real = [], ops.feature_cache_gather
    monkeypatch.setattr(ops, "feature_cache_gather", lambda *a, **k: [calls.append(1), real(*a, **k)][1])
    got = gpu.gather(ind)
    assert len(calls) == 1 and got.dtype == torch.float32 and tuple(got.shape) == (len(ind),) + shape
    assert torch.equal(bits(got), bits(want))
    idx = torch.tensor(ind + ind_pos, dtype=torch.int64, device=dev)
    n = len(ind)
    out = torch.empty(n, L, dtype=torch.float32, device=dev)
    out.view(torch.uint8).fill_(0xFF)
    assert real(gpu.data, idx[:n], None, out=out) is out
    assert torch.equal(bits(out), bits(want.reshape(n, L)))
    # the paired call: its bits and its single allocation are what they were
    a, b = gpu.gather(ind, ind_pos)
    assert len(calls) == 2 and b.data_ptr() == a.data_ptr() + a.numel() * 4
    assert a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
    assert torch.equal(bits(a), bits(want)) and torch.equal(bits(b), bits(want_pos))


# ---------------------------------------------------------------------------------------------------------------- fit
TRAIN_SIZES = [(40, 40), (44, 48), (52, 40), (40, 56)] * 4                      # (width, height): 16 images, 8 batches of 2 an epoch
VAL_SIZES = [(32, 32), (36, 40), (48, 32), (33, 35), (40, 40)]
FIT = dict(dataset_name="directory", dir_dataset_n_classes=N_CLASSES, res=40, dim=70, feature_samples=5, max_steps=4, val_freq=2, batch_size=BATCH,
           scalar_log_freq=1, num_workers=0, num_neighbors=3, use_depth=False, depth_feat_correlation_loss=False, depth_sampling="none",
           crop_type=None, loader_crop_type="center")


def _val_lines(out_dir):
    return [l for l in (json.loads(l) for l in open(os.path.join(out_dir, "log.jsonl"))) if "val" in l]


def _fit(root, out_dir, dev, val_cache):
    from depthg_amd import data, train
    from depthg_amd.segmenter import UnsupervisedSegmenter
    cfg = train.build_cfg({**FIT, **({"dg_val_feature_cache": "float32"} if val_cache else {})})
    torch.manual_seed(3)
    model = UnsupervisedSegmenter(N_CLASSES, cfg).to(dev)
    model.train()
    train_set = data.DirectoryFolder(root, "train", name="directory", n_classes=N_CLASSES, crop_type=None)
    val_set = data.DirectoryFolder(root, "val", name="directory", n_classes=N_CLASSES, crop_type=None)
    cache = data.build_feature_cache(model.net, val_set, cfg, 32, "center", dtype=torch.float32, device=dev, batch_size=BATCH,
                                     image_set="val") if val_cache else None
    train_batches = data.ContrastiveBatches(train_set, cfg, "train", 40, "center", BATCH, shuffle=True, generator=torch.Generator().manual_seed(0),
                                            pos=True, return_depth=False, device=dev)
    val_batches = data.ContrastiveBatches(val_set, cfg, "val", 32, "center", BATCH, shuffle=False, pos=False, return_depth=False, device=dev,
                                          feature_cache=cache)
    assert len(train_batches) == 8 and len(val_batches) == 3
    calls, real = [], model.net._backbone
    model.net._backbone = lambda *a, **k: [calls.append(bool(model.net.training)), real(*a, **k)][1]
    torch.manual_seed(7)
    state = train.fit(model, train_batches, val_batches, cfg, out_dir, save_checkpoint=lambda m, p: None)
    torch.cuda.synchronize()
    return state, calls


def test_fit_logs_the_same_val_lines_from_a_float32_cache(tmp_path, dev):
    root = str(tmp_path / "data")
    DF.make_directory(root, sizes=TRAIN_SIZES, split="train", n_classes=N_CLASSES)
    DF.make_directory(root, sizes=VAL_SIZES, split="val", n_classes=N_CLASSES, seed=2)
    DF.write_nns(root, "directory", "train", None, 40, len(TRAIN_SIZES))
    plain, plain_calls = _fit(root, str(tmp_path / "plain"), dev, False)
    cached, cached_calls = _fit(root, str(tmp_path / "cached"), dev, True)
    assert plain["steps"] == cached["steps"] == 4 and plain["val_steps"] == cached["val_steps"] == [2, 4]
    # eval-mode backbone calls: three per validation without the cache, none with it (the training steps' calls are in training mode)
    assert plain_calls.count(False) == 6 and cached_calls.count(False) == 0 and plain_calls.count(True) == cached_calls.count(True) > 0
    a, b = _val_lines(str(tmp_path / "plain")), _val_lines(str(tmp_path / "cached"))
    print("val lines, plain: ", a)
    print("val lines, cached:", b)
    assert len(a) == 2 and [l["step"] for l in a] == [2, 4] and "test/cluster/mIoU" in a[0]["val"]
    assert a == b


GRAPH_SOURCE = [(40, 40), (44, 48), (52, 40), (40, 56)] * 4                     # 16 images: 8 steps of 2 an epoch, so val_freq = 2 holds


def _graph_fit(out_dir, dev, val_cache):
    from depthg_amd import data, train
    from depthg_amd.epoch import DeviceEpoch
    from depthg_amd.graph_step import GraphedTrainStep
    from depthg_amd.segmenter import UnsupervisedSegmenter
    over = dict(dim=70, feature_samples=5, dg_feature_cache="float32", dg_graph_safe=True, dg_fused_adam=True, dg_graph_step=True, hist_freq=None,
                max_steps=4, val_freq=2, scalar_log_freq=1, batch_size=BATCH, num_workers=0, num_neighbors=3)
    cfg = train.build_cfg({**over, **({"dg_val_feature_cache": "float32"} if val_cache else {})})
    torch.manual_seed(3)
    seg = UnsupervisedSegmenter(N_CLASSES, cfg).to(dev)
    seg.train()
    ds = MemorySet(make_samples(GRAPH_SOURCE, labels=True, depth="bytes", n_label=6), **CROPPED)
    val_ds = MemorySet(make_samples(VAL_SIZES, labels=True, depth=None, n_label=6, seed=5), **CROPPED)
    samples = data.build_sample_cache(ds, cfg, 40, "center", True, dev, 0, image_set="train")
    feats = data.build_feature_cache(seg.net, ds, cfg, 40, "center", dtype=torch.float32, device=dev, batch_size=len(ds))
    val_feats = data.build_feature_cache(seg.net, val_ds, cfg, 32, "center", dtype=torch.float32, device=dev, batch_size=BATCH,
                                         image_set="val") if val_cache else None
    val_batches = data.ContrastiveBatches(val_ds, cfg, "val", 32, "center", BATCH, shuffle=False, pos=False, return_depth=False, device=dev,
                                          feature_cache=val_feats)
    torch.manual_seed(7)
    ep = DeviceEpoch(case(len(ds), 6)[1], BATCH, 3, dev, shuffle=True, generator=torch.Generator().manual_seed(5))
    assert ep.steps_per_epoch == 8
    wrapper = GraphedTrainStep(seg, ep, samples, feats, strict=True)
    flags, real = [], wrapper.step
    wrapper.step = lambda: [real(), flags.append(bool(wrapper.graphed))][0]
    state = train.fit(seg, None, val_batches, cfg, out_dir, save_checkpoint=lambda m, p: None, graph_step=wrapper)
    torch.cuda.synchronize()
    return state, wrapper.captures, flags


def test_graphed_fit_keeps_its_recording_across_validations(tmp_path, dev):
    plain, plain_captures, plain_flags = _graph_fit(str(tmp_path / "plain"), dev, False)
    cached, cached_captures, cached_flags = _graph_fit(str(tmp_path / "cached"), dev, True)
    assert plain["val_steps"] == cached["val_steps"] == [2, 4]
    assert plain_captures == cached_captures == 1
    assert plain_flags == cached_flags == [False, True, True, True]
    assert len(_val_lines(str(tmp_path / "cached"))) == 2


# ---------------------------------------------------------------------------------------------------------------- train command
CMD_SIZES = [(120, 112), (112, 130), (128, 128), (150, 112), (112, 112), (140, 120), (113, 127), (131, 117)]


def test_train_command_with_val_feature_cache(tmp_path):
    """Three steps of `python -m depthg_amd.train --val-feature-cache float16 --sample-cache --feature-cache float16` on eight small
    images: the val cache is built behind the train one, at 320 x 320, and the val sample cache is filled from the same pass."""
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    DF.make_directory(root, sizes=CMD_SIZES, split="train", n_classes=5)
    DF.make_directory(root, sizes=CMD_SIZES[:4], split="val", n_classes=5, seed=2)
    args = ["--data-dir", root, "--out", out, "--dataset", "directory", "--precompute-knns", "--val-feature-cache", "float16", "--sample-cache",
            "--feature-cache", "float16", "res=112", "dim=70", "max_steps=3", "val_freq=2", "batch_size=2", "scalar_log_freq=1", "num_workers=2",
            "crop_type=~", "loader_crop_type=center", "num_neighbors=3", "use_depth=False", "depth_feat_correlation_loss=False",
            "depth_sampling=none", "dir_dataset_n_classes=5"]
    run = subprocess.run([sys.executable, "-m", "depthg_amd.train"] + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "3 step(s), 1 validation(s)" in run.stdout and "val feature cache built and saved to" in run.stdout
    assert run.stdout.index("feature cache built and saved to") < run.stdout.index("val feature cache built and saved to")
    files = sorted(f for f in os.listdir(root) if f.startswith("feature_cache_"))
    assert len(files) == 2 and "_train_center_112_8_float16.pt" in files[0] and "_val_center_320_4_float16.pt" in files[1], files
    assert os.path.getsize(os.path.join(root, files[1])) > 4 * 384 * 40 * 40 * 2
    assert len([f for f in os.listdir(root) if f.startswith("sample_cache_")]) == 2
    vals = _val_lines(out)
    assert len(vals) == 1 and vals[0]["step"] == 3 and "test/cluster/mIoU" in vals[0]["val"]
