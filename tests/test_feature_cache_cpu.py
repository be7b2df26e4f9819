"""The frozen-backbone feature cache on the CPU (depthg_amd/feature_cache.py, data.build_feature_cache): the two exports, the plain
torch route the kernels are held to (index_copy_, index_select, torch's casts), every refusal, the metadata check of save / load, and
one pass over the stub folders with a tiny backbone.  (The head has no CPU route - ops refuses CPU tensors - so the equality of
forward_pair_features with forward_pair is tests/test_gpu_feature_cache.py's.)"""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import data_folders as DF
from conftest import ROOT
from feature_cache_cases import exact_widen, feature_rows, special_values

DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_exports_and_signatures():
    import depthg_amd
    from depthg_amd import _lib, data, feature_cache, ops
    assert depthg_amd.FeatureCache is feature_cache.FeatureCache and depthg_amd.build_feature_cache is data.build_feature_cache
    for name in ("feature_cache", "FeatureCache", "build_feature_cache"):
        assert name in depthg_amd.__all__
    lib = _lib.load()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["dg_featcache_put"] == (ctypes.c_int, [vp, i32, i64, i64, vp, vp, i64, vp])
    assert _lib.SIGNATURES["dg_featcache_gather"] == (ctypes.c_int, [vp, i32, i64, i64, vp, vp, i64, vp, vp])
    for name in ("dg_featcache_put", "dg_featcache_gather"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    assert "int dg_featcache_put(void* cache, int32_t dtype, int64_t N, int64_t L, const float* src, const int64_t* idx, int64_t n," in header
    assert "int dg_featcache_gather(const void* cache, int32_t dtype, int64_t N, int64_t L, const int64_t* idx_a, const int64_t* idx_b, int64_t n," in header
    assert callable(ops.feature_cache_put) and callable(ops.feature_cache_gather)
    # the entries refuse bad arguments before they would launch anything (no GPU is touched)
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, vp)
    assert lib.dg_featcache_put(p, 3, 1, 8, p, p, 1, None) == -1 and b"dtype" in lib.dg_last_error()
    assert lib.dg_featcache_put(p, 0, 0, 8, p, p, 1, None) == -1
    assert lib.dg_featcache_gather(p, 1, 1, 8, p, None, 70000, p, None) == -2 and b"rows" in lib.dg_last_error()
    assert lib.dg_featcache_gather(None, 1, 1, 8, p, None, 1, p, None) == -1
    assert lib.dg_featcache_gather(p, 0, 1, 8, p, None, 0, p, None) == 0                 # n == 0: nothing to do
    from depthg_amd.segmenter import default_segmenter_cfg
    assert default_segmenter_cfg().dg_feature_cache is None


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float16", "bfloat16"])
def test_cpu_route_round_trip(dtype):
    from depthg_amd import FeatureCache
    C, h, w, N = 3, 5, 7, 6
    cache = FeatureCache(N, C, h, w, dtype=dtype, device="cpu")
    assert cache.nbytes == N * C * h * w * {torch.float32: 4, torch.float16: 2, torch.bfloat16: 2}[dtype]
    assert cache.filled.dtype == np.bool_ and not cache.filled.any() and cache.meta["n_images"] == N
    x = feature_rows(4, C, h, w)
    assert special_values().numel() <= C * h * w
    cache.put([5, 0, 3, 2], x)
    assert cache.filled.tolist() == [True, False, True, True, False, True]
    want = x.to(dtype).float()
    got = cache.gather(torch.tensor([0, 5, 2, 3]))
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, C, h, w)
    assert torch.equal(_bits(got), _bits(want[[1, 0, 3, 2]]))
    if dtype == torch.float32:
        assert torch.equal(_bits(got), _bits(x[[1, 0, 3, 2]]))
    else:                                   # the special values did exercise the cast: rounding changed some, NaN and infinity survived
        assert not torch.equal(_bits(want), _bits(x)) and torch.isnan(got).any() and torch.isinf(got).any()
    # two lists: views of one allocation, rows of `ind` then rows of `ind_pos`; repeats are legal, inside a list and between them
    a, b = cache.gather([0, 0, 5], [5, 3, 0])
    assert a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and b.data_ptr() == a.data_ptr() + a.numel() * 4
    assert torch.equal(_bits(a), _bits(want[[1, 1, 0]])) and torch.equal(_bits(b), _bits(want[[0, 2, 1]]))
    # an overwrite replaces the row and nothing else
    cache.put([3], x[:1])
    assert torch.equal(_bits(cache.gather([3, 2])), _bits(want[[0, 3]]))


def test_cpu_gather_is_the_exact_widening():
    """What the GPU tests hold k_fc_gather to (feature_cache_cases.exact_widen) is what FeatureCache's CPU route returns: rows whose
    element count is a multiple of eight - torch widens every float16 of them in whole vectors - come back with exact_widen's bits,
    NaN included, for all three types; and exact_widen is torch's own cast on everything that is no NaN."""
    from depthg_amd import FeatureCache
    s = special_values()
    k = s.numel() // 8 * 8
    for dtype in DTYPES:
        cache = FeatureCache(3, k // 8, 2, 4, dtype=dtype, device="cpu")
        rows = torch.stack([s[:k], s[:k].flip(0)]).reshape(2, k // 8, 2, 4)
        cache.put([2, 0], rows)
        got = cache.gather([0, 2])
        assert torch.isnan(got).any()
        assert torch.equal(_bits(got), _bits(exact_widen(rows[[1, 0]].to(dtype))))
        finite = s[~torch.isnan(s)].to(dtype)
        assert torch.equal(_bits(exact_widen(finite)), _bits(finite.float()))


def test_refusals():
    from depthg_amd import FeatureCache
    cache = FeatureCache(4, 2, 3, 3, device="cpu")
    x = torch.randn(2, 2, 3, 3)
    with pytest.raises(IndexError, match=r"holds 4, outside \[0, 4\)"):
        cache.put([1, 4], x)
    with pytest.raises(IndexError, match="holds -1"):
        cache.put([-1, 2], x)
    with pytest.raises(ValueError, match="names row 2 more than once"):
        cache.put([2, 2], x)
    with pytest.raises(ValueError, match="put of 3 indices"):
        cache.put([0, 1, 2], x)
    with pytest.raises(ValueError, match="wants image_feat"):
        cache.put([0, 1], torch.randn(2, 2, 3, 4))
    with pytest.raises(ValueError, match="integer"):
        cache.put(torch.tensor([0.0, 1.0]), x)
    assert not cache.filled.any()                              # a refused put stored nothing
    cache.put([0, 1], x)
    with pytest.raises(IndexError, match="`ind` holds 7"):
        cache.gather([0, 7])
    with pytest.raises(IndexError, match="`ind_pos` holds -2"):
        cache.gather([0, 1], [1, -2])
    with pytest.raises(ValueError, match="row 3 of `ind` was never put"):
        cache.gather([0, 3])
    with pytest.raises(ValueError, match="row 2 of `ind_pos` was never put"):
        cache.gather([0, 1], [1, 2])
    with pytest.raises(ValueError, match="2 indices and 1 positives"):
        cache.gather([0, 1], [1])
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        FeatureCache(4, 2, 3, 3, dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError):
        FeatureCache(0, 2, 3, 3, device="cpu")


def test_save_load_and_metadata(tmp_path):
    from depthg_amd import FeatureCache
    meta = dict(model_type="vit_small", dino_patch_size=8, dino_feat_type="feat", res=16, loader_crop_type="center", dataset_name="x_None")
    cache = FeatureCache(3, 2, 2, 2, dtype=torch.float16, device="cpu", meta=meta)
    x = feature_rows(2, 2, 2, 2, seed=3)
    cache.put([2, 0], x)
    path = str(tmp_path / "cache.pt")
    cache.save(path)
    back = FeatureCache.load(path, "cpu", expect_meta={**meta, "n_images": 3})
    assert back.dtype == torch.float16 and back.shape == (2, 2, 2) and back.meta == cache.meta and back.filled.tolist() == [True, False, True]
    assert torch.equal(_bits(back.gather([0, 2])), _bits(cache.gather([0, 2])))
    with pytest.raises(ValueError, match="row 1"):
        back.gather([1])
    with pytest.raises(ValueError) as e:
        FeatureCache.load(path, "cpu", expect_meta={**meta, "res": 224, "dino_feat_type": "KK"})
    assert "res = 16 (expected 224)" in str(e.value) and "dino_feat_type" in str(e.value) and "model_type" not in str(e.value)
    with pytest.raises(ValueError, match="n_images = 3"):
        FeatureCache.load(path, "cpu", expect_meta={"n_images": 4})


def _tiny_net(cfg):
    from depthg_amd.segmenter import StandInFeaturizer
    torch.manual_seed(0)
    return StandInFeaturizer(8, cfg, backbone=torch.nn.Conv2d(3, 384, 8, stride=8))


@pytest.mark.parametrize("crop_type", ["center", None])
def test_build_feature_cache_on_folders(tmp_path, crop_type):
    from depthg_amd import data
    from depthg_amd.segmenter import default_segmenter_cfg
    root, res = str(tmp_path), 16
    DF.make_directory(root, n_classes=5)
    ds = data.DirectoryFolder(root, "train", name="directory", n_classes=5, crop_type=None)
    cfg = default_segmenter_cfg(res=res)
    net = _tiny_net(cfg)
    cache = data.build_feature_cache(net, ds, cfg, res, crop_type, dtype=torch.float32, device="cpu", batch_size=3, num_workers=2)
    assert cache.n_images == len(DF.SIZES) and cache.shape == (384, 2, 2) and cache.filled.all() and cache.dtype == torch.float32
    assert cache.meta == {"n_images": 8, "model_type": "vit_small", "dino_patch_size": 8, "dino_feat_type": "feat", "res": 16,
                          "loader_crop_type": crop_type, "dataset_name": "directory_None", "pretrained_weights": None}
    # row i is the backbone on image i through the loader's plain chain
    samples = [ds.load(i) for i in (6, 1)]
    img = data.prepare_samples(ds, samples, res, crop_type, "cpu", False)[0]
    with torch.no_grad():
        want = net._backbone(img)[0]
    assert torch.equal(_bits(cache.gather([6, 1])), _bits(want))
    # and the pipeline hands the rows out with every batch
    DF.write_nns(root, "directory", "train", None, res, len(DF.SIZES))
    batches = data.ContrastiveBatches(ds, SimpleNamespace(model_type=DF.MODEL_TYPE, res=res, num_neighbors=3), "train", res, crop_type, 3,
                                      device="cpu", feature_cache=cache)
    batch = next(iter(batches))
    assert tuple(batch["image_feat"].shape) == (3, 384, 2, 2) and tuple(batch["image_feat_pos"].shape) == (3, 384, 2, 2)
    with torch.no_grad():
        assert torch.equal(_bits(batch["image_feat"]), _bits(net._backbone(batch["img"])[0]))
        assert torch.equal(_bits(batch["image_feat_pos"]), _bits(net._backbone(batch["img_pos"])[0]))


def test_build_feature_cache_refusals(tmp_path):
    from depthg_amd import data
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    root, res = str(tmp_path), 16
    DF.make_directory(root, n_classes=5)
    DF.write_nns(root, "directory", "train", None, res, len(DF.SIZES))
    ds = data.DirectoryFolder(root, "train", name="directory", n_classes=5, crop_type=None)
    cfg = default_segmenter_cfg(res=res)
    net = _tiny_net(cfg)
    with pytest.raises(ValueError, match="random"):
        data.build_feature_cache(net, ds, cfg, res, "random", device="cpu")
    with pytest.raises(ValueError, match="out of scope"):
        data.build_feature_cache(net, ds, default_segmenter_cfg(res=res, arch="dino_depth"), res, "center", device="cpu")
    cache = data.build_feature_cache(net, ds, cfg, res, "center", dtype="bfloat16", device="cpu", batch_size=8)
    assert cache.dtype == torch.bfloat16
    loader_cfg = SimpleNamespace(model_type=DF.MODEL_TYPE, res=res, num_neighbors=3)
    with pytest.raises(ValueError, match="random"):
        data.ContrastiveBatches(ds, loader_cfg, "train", res, "random", 2, device="cpu", feature_cache=cache)
    # the step's construction refuses the one LHP strategy that reads the attention map
    with pytest.raises(ValueError, match="attention map"):
        UnsupervisedSegmenter(5, default_segmenter_cfg(dg_feature_cache="float32", lhp=True, propagation_strategy="attn"))
