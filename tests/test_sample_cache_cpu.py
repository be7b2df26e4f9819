"""The device-resident sample cache without a GPU: the library's two exports, the class's plain torch route against data._cpu_chain bit
for bit, its refusals, save / load, and data.build_sample_cache / ContrastiveBatches(sample_cache=...) on stub folders against the
pipeline without a cache."""
import ctypes
import os

import numpy as np
import pytest
import torch

import data_folders as DF
from sample_cache_cases import CROPPED, DIRECTORY, MemorySet, chain, make_samples, same_bits

SIZES = [(37, 53), (301, 200), (16, 16), (53, 37), (20, 64)]


def test_exports_and_signatures():
    from depthg_amd import _lib
    lib = _lib.load()
    for name in ("dg_samplecache_put", "dg_samplecache_gather"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int
    assert len(_lib.SIGNATURES["dg_samplecache_put"][1]) == 15 and len(_lib.SIGNATURES["dg_samplecache_gather"][1]) == 19


def _cache_for(ds, n, res, want_depth, device="cpu"):
    from depthg_amd import SampleCache
    return SampleCache(n, res, res, ds.has_labels, want_depth, ds.label_offset if ds.has_labels else 0, -1, ds.mask_rule, device=device)


@pytest.mark.parametrize("rules", [CROPPED, DIRECTORY], ids=["bool-mask", "float-mask"])
@pytest.mark.parametrize("labels,depth", [(True, "bytes"), (True, "plane"), (True, None), (False, None), (False, "bytes")],
                         ids=["label+depth", "label+plane", "label", "bare", "depth"])
@pytest.mark.parametrize("res,crop", [(16, "center"), (20, None), (4, "center")])
def test_cpu_route_equals_the_cpu_chain(res, crop, labels, depth, rules):
    samples = make_samples(SIZES, labels=labels, depth=depth)
    ds = MemorySet(samples, **rules)
    want_depth = depth is not None
    cache = _cache_for(ds, len(samples) + 2, res, want_depth)
    cache.data.fill_(7)
    rows = [5, 0, 3, 6, 2]
    cache.put(rows, samples, res, crop)
    assert cache.filled.tolist() == [True, False, True, True, False, True, True]
    assert bool((cache.data[[1, 4]] == 7).all())                                   # a put leaves the other rows alone
    ref = chain(ds, samples, res, crop, want_depth)
    for k, row in enumerate(rows):                                                 # sample by sample
        got = cache.gather([row])
        for g, r in zip(got, ref):
            assert same_bits(g, None if r is None else r[k:k + 1])
    # a batch and its positives: the batch first, the positives behind it; indices repeat inside a list and between the two
    inds, pos = [5, 5, 2], [2, 0, 5]
    got = cache.gather(inds, pos)
    order = [rows.index(i) for i in inds + pos]
    for g, r in zip(got, ref):
        assert same_bits(g, None if r is None else r[order])
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and tuple(got[0].shape) == (6, 3, res, res)
    assert got[2].dtype == (torch.bool if rules is CROPPED else torch.float32)
    if not labels:
        assert bool((got[1] == -1).all())
    if depth == "plane":
        assert bool((got[3] == 255.0).all())


def test_refusals():
    from depthg_amd import SampleCache, ops
    samples = make_samples(SIZES)
    ds = MemorySet(samples, **CROPPED)
    with pytest.raises(ValueError, match="multiple of 4"):
        SampleCache(4, 18, 18, True, True, -1, -1, ops.BATCH_MASK_BOOL_IGNORED, device="cpu")
    with pytest.raises(ValueError, match="mask rule"):
        SampleCache(4, 16, 16, True, True, -1, -1, 2, device="cpu")
    cache = _cache_for(ds, 5, 16, True)
    with pytest.raises(ValueError, match="'center' or None"):
        cache.put([0], samples[:1], 16, "random")
    with pytest.raises(ValueError, match="the cache's rows hold 16 x 16"):           # outputs that do not share the cache's (H, W)
        cache.put([0, 1], samples[:2], 20, None)
    with pytest.raises(ValueError, match="carries no label but the cache has a label plane"):
        cache.put([0], make_samples(SIZES[:1], labels=False), 16, "center")
    bare = _cache_for(MemorySet(make_samples(SIZES, labels=False, depth=None), **DIRECTORY), 5, 16, False)
    with pytest.raises(ValueError, match="carries a label but the cache has no label plane"):
        bare.put([0], make_samples(SIZES[:1], labels=True, depth=None), 16, "center")
    with pytest.raises(ValueError, match="depth was asked for"):
        cache.put([0], make_samples(SIZES[:1], depth=None), 16, "center")
    with pytest.raises(ValueError, match="more than once"):
        cache.put([1, 1], samples[:2], 16, "center")
    with pytest.raises(ValueError, match="2 indices got 1 samples"):
        cache.put([1, 2], samples[:1], 16, "center")
    with pytest.raises(IndexError, match="outside"):
        cache.put([5], samples[:1], 16, "center")
    assert not cache.filled.any()                                                   # a refused put stores nothing
    cache.put([1], samples[:1], 16, "center")
    with pytest.raises(ValueError, match="row 3 of `inds_pos` was never put"):
        cache.gather([1], [3])
    with pytest.raises(ValueError, match="1 indices and 2 positives"):
        cache.gather([1], [1, 1])
    with pytest.raises(IndexError):
        cache.gather([-1])


def test_allocation_failure_names_the_bytes(monkeypatch):
    from depthg_amd import SampleCache, ops

    def refuse(*a, **k):
        raise torch.OutOfMemoryError("no room")
    monkeypatch.setattr(torch, "empty", refuse)
    with pytest.raises(torch.OutOfMemoryError, match=str(1000 * 5 * 224 * 224) + " bytes"):
        SampleCache(1000, 224, 224, True, True, -1, -1, ops.BATCH_MASK_BOOL_IGNORED, device="cpu")


def test_save_load_and_metadata(tmp_path):
    from depthg_amd import SampleCache, data
    samples = make_samples(SIZES)
    ds = MemorySet(samples, **CROPPED)
    cache = data.build_sample_cache(ds, None, 16, "center", device="cpu", image_set="train", batch_size=2)
    assert ds.loads == len(samples) and cache.filled.all() and cache.with_depth and cache.nbytes == 5 * 5 * 16 * 16
    meta = data.sample_cache_meta(ds, "train", 16, "center", True)
    assert cache.meta == meta and set(meta) == {"dataset_name", "split", "res", "loader_crop_type", "n_images", "has_labels", "depth_type"}
    path = str(tmp_path / os.path.basename(data.sample_cache_path(str(tmp_path), meta)))
    cache.save(path)
    back = SampleCache.load(path, "cpu", expect_meta=meta)
    assert torch.equal(back.data, cache.data) and back.filled.all() and back.meta == cache.meta
    assert (back.has_labels, back.with_depth, back.label_offset, back.fill, back.mask_rule) == (True, True, -1, -1, ds.mask_rule)
    for g, r in zip(back.gather([4, 0], [1, 4]), cache.gather([4, 0], [1, 4])):
        assert same_bits(g, r)
    for key, other in (("res", 20), ("split", "val"), ("loader_crop_type", None), ("n_images", 6), ("depth_type", None), ("has_labels", False)):
        with pytest.raises(ValueError, match=key):
            SampleCache.load(path, "cpu", expect_meta={**meta, key: other})
    with pytest.raises(ValueError, match="'center' or None"):
        data.build_sample_cache(ds, None, 16, "random", device="cpu")


# ---------------------------------------------------------------------------------------------------------------- pipelines
FOLDER_SIZES = [(37, 23), (23, 37), (64, 64), (50, 20), (30, 25), (64, 64), (23, 37)]


def _cfg(**over):
    from depthg_amd.segmenter import default_segmenter_cfg
    return default_segmenter_cfg(**{**dict(model_type=DF.MODEL_TYPE, num_neighbors=3), **over})


def _counted(ds):
    real, ds.loads = ds.load, 0

    def load(i):
        ds.loads += 1
        return real(i)
    ds.load = load
    return ds


def _same_batches(plain, cached):
    torch.manual_seed(11)
    want = list(plain)
    torch.manual_seed(11)
    got = list(cached)
    assert len(want) == len(got) and len(want) > 1
    for a, b in zip(want, got):
        assert list(a) == list(b)
        for k in a:
            assert same_bits(a[k], b[k]), k
    return want


@pytest.mark.parametrize("pos", [True, False], ids=["pos", "val"])
def test_cropped_folder_with_depth(tmp_path, pos):
    from depthg_amd import data
    root = str(tmp_path)
    DF.make_cropped(root, sizes=FOLDER_SIZES)
    DF.write_nns(root, "cocostuff27", "train", "five", 16, len(FOLDER_SIZES))
    ds = _counted(data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train", return_depth=True))
    cfg = _cfg(res=16)
    cache = data.build_sample_cache(ds, cfg, 16, "center", True, "cpu", 2)
    assert ds.loads == len(FOLDER_SIZES)
    kw = dict(shuffle=pos, num_workers=2, pos=pos, device="cpu")
    plain = data.ContrastiveBatches(ds, cfg, "train", 16, "center", 3, generator=torch.Generator().manual_seed(5), **kw)
    cached = data.ContrastiveBatches(ds, cfg, "train", 16, "center", 3, generator=torch.Generator().manual_seed(5), sample_cache=cache, **kw)
    want = _same_batches(plain, cached)
    assert set(want[0]) == {"ind", "img", "label", "mask", "depth"} | ({"img_pos", "ind_pos", "label_pos", "mask_pos", "depth_pos"} if pos else set())
    assert tuple(want[0]["label"].shape) == (3, 16, 16) and tuple(want[0]["mask"].shape) == (3, 1, 16, 16) and tuple(want[0]["depth"].shape) == (3, 1, 16, 16)
    before = ds.loads
    for _ in cached:
        pass
    assert ds.loads == before                                                       # no sample is decoded behind the build
    # a pipeline that wants no depth reads the same cache
    nodepth = data.ContrastiveBatches(ds, cfg, "train", 16, "center", 3, return_depth=False, sample_cache=cache, **kw)
    assert "depth" not in next(iter(nodepth))
    for bad, match in ((dict(loader_crop_type="random"), "ONE view"), (dict(res=20), "not built for this pipeline")):
        args = {**dict(res=16, loader_crop_type="center"), **bad}
        with pytest.raises(ValueError, match=match):
            data.ContrastiveBatches(ds, cfg, "train", args["res"], args["loader_crop_type"], 3, sample_cache=cache, **kw)
    short = data.build_sample_cache(MemorySet(make_samples(SIZES), **CROPPED), cfg, 16, "center", True, "cpu", 0)
    with pytest.raises(ValueError, match="holds 5 images"):
        data.ContrastiveBatches(ds, cfg, "train", 16, "center", 3, sample_cache=short, **kw)
    without = data.build_sample_cache(ds, cfg, 16, "center", False, "cpu", 0)
    with pytest.raises(ValueError, match="not built for this pipeline"):
        data.ContrastiveBatches(ds, cfg, "train", 16, "center", 3, return_depth=True, sample_cache=without, **kw)


@pytest.mark.parametrize("labels", [False, True], ids=["unlabelled", "labelled"])
def test_directory_folder(tmp_path, labels):
    from depthg_amd import data
    root = str(tmp_path)
    DF.make_directory(root, sizes=FOLDER_SIZES, labels=labels)
    DF.write_nns(root, "directory", "train", None, 12, len(FOLDER_SIZES))
    ds = _counted(data.DirectoryFolder(root, "train", n_classes=5))
    cfg = _cfg(res=12)
    cache = data.build_sample_cache(ds, cfg, 12, None, None, "cpu", 0)
    assert cache.has_labels == labels and not cache.with_depth and cache.planes == 3 + labels
    kw = dict(shuffle=True, pos=True, device="cpu")
    plain = data.ContrastiveBatches(ds, cfg, "train", 12, None, 4, generator=torch.Generator().manual_seed(2), **kw)
    cached = data.ContrastiveBatches(ds, cfg, "train", 12, None, 4, generator=torch.Generator().manual_seed(2), sample_cache=cache, **kw)
    before = ds.loads
    want = _same_batches(plain, cached)
    assert ds.loads == before + 2 * len(FOLDER_SIZES)                               # the plain pipeline's own decoding, none from the cached one
    assert tuple(want[0]["label"].shape) == ((4, 1, 12, 12) if labels else (4, 12, 12)) and want[0]["mask"].dtype == torch.float32
    assert "depth" not in want[0]


def test_feature_cache_pass_fills_a_sample_cache(tmp_path):
    """build_feature_cache(sample_cache=...) puts the samples it decodes: one decoding pass for both caches.  (A CPU stand-in for the
    featurizer: the pass only needs `_backbone`.)"""
    from depthg_amd import data
    samples = make_samples(SIZES, depth=None)
    ds = MemorySet(samples, **CROPPED)

    class Net:
        model = torch.nn.Identity()
        forward_pair_features = True

        def _backbone(self, img):
            return (img[:, :, ::4, ::4].contiguous(),)

    cfg = _cfg(res=16, dino_patch_size=8)
    filled = data.new_sample_cache(ds, "train", 16, "center", False, "cpu")
    feats = data.build_feature_cache(Net(), ds, cfg, 16, "center", device="cpu", batch_size=2, sample_cache=filled)
    assert ds.loads == len(samples) and filled.filled.all() and feats.filled.all()
    alone = data.build_sample_cache(ds, cfg, 16, "center", False, "cpu", 0)
    assert torch.equal(filled.data, alone.data)
    assert np.array_equal(data.fill_sample_cache(filled, ds, 16, "center").filled, np.ones(5, bool)) and ds.loads == 2 * len(samples)
