"""The validation feature cache on the CPU (train.val_feature_cache, data.ContrastiveBatches(pos=False, feature_cache=...),
UnsupervisedSegmenter.validation_step / evaluate_batch under cfg.dg_val_feature_cache): the file and its metadata, the val
batches, the route behind the backbone and every refusal, on stub folders with a tiny stand-in backbone.  The head and the fused
probe-and-score launch have no CPU route, so both are replaced here by the plain torch statements of what they compute (eval mode:
no dropout) - the cached and the uncached validation then run the same arithmetic on the same features, and what is checked is the
plumbing: which route ran, what it was fed, what came out.  The kernels' side is tests/test_gpu_val_cache.py's."""
import os

import pytest
import torch
import torch.nn.functional as F

import data_folders as DF

N_VAL, N_CLASSES, BATCH = 5, 5, 2
VAL_SIZES = [(330, 325), (400, 320), (320, 360), (350, 350), (321, 333)]          # (width, height): a centre crop of 320 x 320 from each


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cfg(**over):
    from depthg_amd.train import build_cfg
    return build_cfg({"dataset_name": "directory", "dir_dataset_n_classes": N_CLASSES, "batch_size": BATCH, "num_workers": 0, "dim": 16,
                      "use_depth": False, **over})


def _net(cfg):
    from depthg_amd.segmenter import StandInFeaturizer
    torch.manual_seed(0)
    return StandInFeaturizer(cfg.dim, cfg)


def _val_set(root):
    from depthg_amd import data
    return data.DirectoryFolder(root, "val", name="directory", n_classes=N_CLASSES, crop_type=None)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """(root, val set, net, float32 val cache, mirrored float32 cache) - built once; no test changes them."""
    from depthg_amd import data, train
    root = str(tmp_path_factory.mktemp("val_cache"))
    DF.make_directory(root, sizes=VAL_SIZES, split="val", n_classes=N_CLASSES, seed=2)
    cfg = _cfg()
    ds, net = _val_set(root), _net(cfg)
    cache = train.val_feature_cache(cfg, root, "cpu", ds, net, "float32")
    mirrored = data.build_feature_cache(net, ds, cfg, 320, "center", dtype=torch.float32, device="cpu", batch_size=BATCH, image_set="val",
                                        mirrored=True)
    return root, ds, net, cache, mirrored


def _val_batches(ds, cfg, cache, **kw):
    from depthg_amd import data
    return data.ContrastiveBatches(ds, cfg, "val", 320, "center", BATCH, shuffle=False, pos=False, return_depth=False, device="cpu",
                                   feature_cache=cache, **kw)


# ---------------------------------------------------------------------------------------------------------------- the file
def test_val_feature_cache_builds_saves_reloads_and_rebuilds(folders, tmp_path, capsys):
    from depthg_amd import data, train
    from depthg_amd.feature_cache import FeatureCache
    root, ds, net, cache, _ = folders
    assert train.val_view(_cfg()) == (320, "center") and train.val_view(_cfg(model_type="mae")) == (224, "center")
    assert train.val_view(_cfg(dataset_name="voc")) == (320, None)
    assert cache.n_images == N_VAL and cache.shape == (384, 40, 40) and cache.dtype == torch.float32 and cache.filled.all()
    assert cache.nbytes == N_VAL * 384 * 40 * 40 * 4
    assert cache.meta["split"] == "val" and cache.meta["res"] == 320 and cache.meta["loader_crop_type"] == "center" and cache.meta["n_images"] == N_VAL
    files = [f for f in os.listdir(root) if f.startswith("feature_cache_")]
    assert len(files) == 1 and "_val_center_320_5_float32.pt" in files[0], files
    path = os.path.join(root, files[0])
    capsys.readouterr()
    # a second call loads the file: the backbone does not run, the rows are the same bits
    cfg = _cfg()
    counted = _count_backbone(net)
    again = train.val_feature_cache(cfg, root, "cpu", ds, net, "float32")
    assert counted["calls"] == 0 and "val feature cache loaded from" in capsys.readouterr().out
    assert torch.equal(_bits(again.data), _bits(cache.data)) and again.meta == cache.meta
    # a file at the same path whose metadata differ (pretrained_weights is no part of the name) is rebuilt, and says why
    mtime = os.stat(path).st_mtime_ns
    rebuilt = train.val_feature_cache(_cfg(pretrained_weights="other.pth"), root, "cpu", ds, net, "float32")
    out = capsys.readouterr().out
    assert "does not match" in out and "pretrained_weights" in out and "val feature cache built and saved to" in out
    assert counted["calls"] == 3 and rebuilt.meta["pretrained_weights"] == "other.pth" and os.stat(path).st_mtime_ns != mtime
    del net._backbone
    cache.save(path)                                            # (the fixture's file back in place)
    assert FeatureCache.load(path, "cpu", expect_meta=data.feature_cache_meta(cfg, ds, 320, "center", image_set="val")).filled.all()
    # the other storage types have files of their own
    half = train.val_feature_cache(cfg, str(tmp_path), "cpu", ds, net, "bfloat16")
    assert half.dtype == torch.bfloat16 and half.nbytes == cache.nbytes // 2
    assert [f for f in os.listdir(str(tmp_path))] == [files[0].replace("float32", "bfloat16")]


def test_a_train_cache_file_is_not_taken_for_the_val_split(folders, tmp_path, capsys):
    """Split, resolution, crop and image count all take part in the match; a train-form file (no split in its metadata) put at the
    val file's path is refused and rebuilt."""
    from depthg_amd import data, train
    from depthg_amd.feature_cache import FeatureCache
    root, ds, net, cache, mirrored = folders
    cfg = _cfg()
    val_meta = data.feature_cache_meta(cfg, ds, 320, "center", image_set="val")
    train_meta = data.feature_cache_meta(cfg, ds, 320, "center")
    assert "split" not in train_meta and val_meta == {**train_meta, "split": "val"}
    val_path = data.feature_cache_path(str(tmp_path), val_meta, "val", "float32")
    assert val_path != data.feature_cache_path(str(tmp_path), train_meta, "train", "float32")
    assert val_path != data.feature_cache_path(str(tmp_path), mirrored.meta, "val", "float32") and mirrored.meta["mirrored"] is True
    # the train split's form of the very same view, saved where the val file would be
    as_train = FeatureCache(N_VAL, *cache.shape, dtype=torch.float32, device="cpu", meta=train_meta)
    as_train.put(list(range(N_VAL)), cache.gather(list(range(N_VAL))))
    as_train.save(val_path)
    with pytest.raises(ValueError, match=r"split = None \(expected 'val'\)"):
        FeatureCache.load(val_path, "cpu", expect_meta=val_meta)
    capsys.readouterr()
    got = train.val_feature_cache(cfg, str(tmp_path), "cpu", ds, net, "float32")
    out = capsys.readouterr().out
    assert "does not match" in out and "split" in out and "built and saved" in out and got.meta["split"] == "val"
    # every part of the view is matched on
    for key, other in (("split", "train"), ("res", 224), ("loader_crop_type", None), ("n_images", N_VAL + 1)):
        with pytest.raises(ValueError, match=key):
            FeatureCache.load(val_path, "cpu", expect_meta={**val_meta, key: other})


# ---------------------------------------------------------------------------------------------------------------- the batches
def test_val_batches_carry_image_feat(folders):
    root, ds, net, cache, _ = folders
    batches = _val_batches(ds, _cfg(), cache)
    assert len(batches) == 3
    seen = []
    for batch in batches:
        seen.append(batch["img"].shape[0])
        assert "image_feat_pos" not in batch and "img_pos" not in batch
        feat = batch["image_feat"]
        assert feat.dtype == torch.float32 and tuple(feat.shape) == (batch["img"].shape[0], 384, 40, 40)
        with torch.no_grad():
            assert torch.equal(_bits(feat), _bits(net._backbone(batch["img"])[0]))
    assert seen == [2, 2, 1]                                   # the short last batch is kept
    # without a cache the val batches are what they were
    plain = next(iter(_val_batches(ds, _cfg(), None)))
    assert "image_feat" not in plain


# ---------------------------------------------------------------------------------------------------------------- the routes
def _torch_head(cluster1, cluster2, image_feat, training, feats_dropout, p=0.1, *args, **kwargs):
    """head.run_head in eval mode (src/modules.py:122-137): code = cluster1(f) + cluster2(f), feats = f."""
    assert not training
    x = image_feat.contiguous()
    return cluster1(x) + (cluster2(x) if cluster2 is not None else 0), x


def _torch_predict(code, label, lin_w, lin_b, clusters, code_flip=None, stats_lin=None, stats_clu=None, n_store=0):
    """ops.segment_predict as the reference's chain (src/train_segmentation.py:471-499)."""
    if code_flip is not None:
        code = (code + code_flip.flip(dims=[3])) / 2
    H, W = label.shape[-2:]
    n = lin_w.shape[0]
    up = F.interpolate(code, (H, W), mode="bilinear", align_corners=False)
    lin = F.conv2d(up, lin_w.reshape(n, -1, 1, 1), lin_b).argmax(1)
    clu = torch.einsum("bchw,nc->bnhw", F.normalize(up, dim=1), F.normalize(clusters, dim=1)).argmax(1)
    lab = label.reshape(-1, H, W).to(torch.int64)
    for stats, pred in ((stats_lin, lin), (stats_clu, clu)):
        if stats is not None:
            ok = (lab >= 0) & (lab < n) & (pred >= 0) & (pred < n)
            stats += torch.bincount(n * pred[ok] + lab[ok], minlength=stats.shape[0] * n).reshape(stats.shape[0], n)
    return (lin[:n_store], clu[:n_store]) if n_store else (None, None)


@pytest.fixture
def torch_routes(monkeypatch):
    from depthg_amd import featurizer, ops
    monkeypatch.setattr(featurizer, "run_head", _torch_head)
    monkeypatch.setattr(ops, "segment_predict", _torch_predict)


def _count_backbone(net):
    """Wrap the featurizer's _backbone: {"calls": n}."""
    counted, real = {"calls": 0}, net._backbone

    def wrapper(*args, **kwargs):
        counted["calls"] += 1
        return real(*args, **kwargs)
    net._backbone = wrapper
    return counted


def _model(**over):
    from depthg_amd.segmenter import UnsupervisedSegmenter
    torch.manual_seed(0)
    model = UnsupervisedSegmenter(N_CLASSES, _cfg(**over))
    model.train()
    return model


def _validate(model, batches):
    outs = [model.validation_step(batch, i) for i, batch in enumerate(batches)]
    assert model.net.training                                   # the mode is restored
    return outs, model.on_validation_epoch_end()


def test_validation_step_from_the_cache_runs_no_backbone(folders, torch_routes):
    root, ds, _, cache, _ = folders
    plain, cached = _model(), _model(dg_val_feature_cache="float32")
    n_plain, n_cached = _count_backbone(plain.net), _count_backbone(cached.net)
    want, want_metrics = _validate(plain, _val_batches(ds, plain.cfg, None))
    got, got_metrics = _validate(cached, _val_batches(ds, cached.cfg, cache))
    assert n_plain["calls"] == 3 and n_cached["calls"] == 0
    assert len(want) == len(got) == 3
    for a, b in zip(want, got):
        assert set(a) == set(b) == {"img", "linear_preds", "cluster_preds", "label"}
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        assert a["img"].shape[0] == min(a["label"].shape[0], 5) and a["linear_preds"].shape[-2:] == (320, 320)
    assert want_metrics == got_metrics and set(want_metrics) >= {"test/cluster/mIoU", "test/linear/Accuracy", "test/linear/MaxmIoU"}
    # a batch without the key takes the backbone, as ever
    cached.validation_step(next(iter(_val_batches(ds, cached.cfg, None))), 0)
    assert n_cached["calls"] == 1


def test_without_the_cfg_key_a_batch_with_image_feat_runs_the_backbone(folders, torch_routes):
    root, ds, _, cache, _ = folders
    model = _model()
    assert model.cfg.dg_val_feature_cache is None
    counted = _count_backbone(model.net)
    batch = next(iter(_val_batches(ds, model.cfg, cache)))
    want = model.validation_step({k: v for k, v in batch.items() if k != "image_feat"}, 0)
    got = model.validation_step({**batch, "image_feat": torch.full_like(batch["image_feat"], float("nan"))}, 0)
    assert counted["calls"] == 2
    assert all(torch.equal(want[k], got[k]) for k in want)
    model.evaluate_batch({**batch, "image_feat": torch.full_like(batch["image_feat"], float("nan"))}, flip=True)
    assert counted["calls"] == 4                                # both passes of the flip route


def test_evaluate_batch_from_the_two_caches(folders, torch_routes):
    root, ds, _, cache, mirrored = folders
    plain, cached = _model(), _model(dg_val_feature_cache="float32")
    n_cached = _count_backbone(cached.net)
    for batch in _val_batches(ds, plain.cfg, cache):
        ind = batch["ind"].tolist()
        both = {**batch, "image_feat_flip": mirrored.gather(ind)}
        for flip, b in ((True, both), (False, batch)):
            want, got = plain.evaluate_batch(batch, flip=flip), cached.evaluate_batch(b, flip=flip)
            assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    assert n_cached["calls"] == 0
    assert torch.equal(plain.test_linear_metrics.stats, cached.test_linear_metrics.stats)
    assert torch.equal(plain.test_cluster_metrics.stats, cached.test_cluster_metrics.stats)
    assert int(plain.test_linear_metrics.stats.sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- the refusals
def test_refusals(folders, torch_routes):
    from depthg_amd import data
    root, ds, net, cache, mirrored = folders
    # arch "dino_depth": at construction
    with pytest.raises(ValueError, match="leave cfg.dg_val_feature_cache unset"):
        _model(dg_val_feature_cache="float32", arch="dino_depth")
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        _model(dg_val_feature_cache="float64")
    # a non-deterministic val crop: where the pipeline and the cache are made
    with pytest.raises(ValueError, match="use 'center' or None"):
        data.ContrastiveBatches(ds, _cfg(), "val", 320, "random", BATCH, pos=False, device="cpu", feature_cache=cache)
    with pytest.raises(ValueError, match="use 'center' or None"):
        data.build_feature_cache(net, ds, _cfg(), 320, "random", device="cpu", image_set="val")
    # a cache whose (C, h, w) is not the featurizer's at the batch's image size
    model = _model(dg_val_feature_cache="float32")
    batch = next(iter(_val_batches(ds, model.cfg, cache)))
    for bad in (batch["image_feat"][:, :, :28, :28], batch["image_feat"][:, :383], batch["image_feat"][:1]):
        with pytest.raises(ValueError, match=r"rebuild it \(train.val_feature_cache"):
            model.validation_step({**batch, "image_feat": bad}, 0)
    assert model.validation_step_outputs == [] and model.net.training
    # flip with image_feat alone: refused, with the fix named
    with pytest.raises(ValueError, match="mirrored=True"):
        model.evaluate_batch(batch, flip=True)
    with pytest.raises(ValueError, match="mirrored=True"):
        model._eval_mode_codes(batch["img"], True, batch["image_feat"])
    with pytest.raises(ValueError, match="rebuild it"):
        model.evaluate_batch({**batch, "image_feat_flip": batch["image_feat"][:, :, :, :39]}, flip=True)
    assert int(model.test_linear_metrics.stats.sum()) == 0
    lin, clu = model.evaluate_batch(batch, flip=False)          # (without the flip pass `image_feat` is enough)
    assert tuple(lin.shape) == (BATCH, 320, 320)


def test_the_train_command_knows_the_flag():
    from depthg_amd import train
    from depthg_amd.segmenter import default_segmenter_cfg
    assert default_segmenter_cfg().dg_val_feature_cache is None
    assert "--val-feature-cache" in train.__doc__ and callable(train.val_feature_cache)
    with pytest.raises(SystemExit):
        train.main(["--data-dir", "x", "--out", "y", "--val-feature-cache", "int8"])
