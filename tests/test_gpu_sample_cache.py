"""The device-resident sample cache on the GPU: gather(put(x)) through k_sc_put / k_sc_gather (dg_sample_cache.hip) against
data.prepare_samples' route on the GPU (dg_batch_prep on the same packed planes and tables) and against the class's plain torch route
on the CPU - img, label, mask and depth bit for bit.  Every kernel case runs with and without poisoned output buffers (ops.POISON,
the DG_POISON=1 hook): an element the kernel left out would be 0xFF bytes.  Then the C entries' refusals and the train command."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import data_folders as DF
from conftest import ROOT
from sample_cache_cases import CROPPED, DIRECTORY, MemorySet, make_samples, same_bits

pytestmark = pytest.mark.gpu

MIXED = [(37, 53), (301, 200), (16, 16)]        # (width, height): smaller and larger than the outputs, and one at 16 x 16 exactly


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(params=[False, True], ids=["plain", "poison"])
def poison(request):
    from depthg_amd import ops
    old = ops.POISON
    ops.POISON = request.param or old
    yield
    ops.POISON = old


def _tables(samples, H, W, res=None, crop=None):
    """[(xs, ys)] per sample: the loader transform's when `res` is given (square outputs), else a plain nearest resize to H x W."""
    from depthg_amd import data
    out = []
    for s in samples:
        h, w = s.image.shape[:2]
        if res is not None:
            xs, ys, size = data.loader_index_tables(w, h, res, crop)
            assert tuple(size) == (H, W)
        else:
            xs, ys = data._pil_nearest_axis(w, W, 0), data._pil_nearest_axis(h, H, 1)
        out.append((xs, ys))
    return out


def _caches(ds, n_rows, H, W, want_depth, dev):
    from depthg_amd import SampleCache
    args = (n_rows, H, W, ds.has_labels, want_depth, ds.label_offset if ds.has_labels else 0, -1, ds.mask_rule)
    return SampleCache(*args, device="cpu"), SampleCache(*args, device=dev)


def _batch_prep(ds, samples, tables, H, W, want_depth, dev):
    """dg_batch_prep on the same planes and tables: what data.prepare_samples launches."""
    from depthg_amd import data, ops
    packed, records, table = data.pack_batch(ds, samples, tables, (H, W), want_depth)
    out = ops.batch_prep(packed, records, table, (H, W), device=dev, mean=ops.IMAGENET_MEAN, std=ops.IMAGENET_STD)
    return out["img"], out["label"], out["mask"], out.get("depth")


# (H, W), res / crop or None (a plain resize to H x W):
#   4 x 4 one lane;  20 x 68 crosses the put's 16 x 64 tile on both axes with a partial last tile;  32 x 16 and 224 x 224: W % 16 == 0,
#   and at 224 x 224 a row's planes span 49 blocks of the gather;  16 x 16 under `None` with sources of equal sizes
OUTPUTS = [((4, 4), 4, "center"), ((20, 68), None, None), ((32, 16), None, None), ((224, 224), 224, "center"), ((16, 16), 16, None),
           ((20, 20), 20, "center")]
PLANES = [(True, "bytes", CROPPED), (True, "plane", CROPPED), (True, None, DIRECTORY), (False, None, DIRECTORY), (False, "bytes", CROPPED)]
PLANE_IDS = ["label+depth-bool", "label+plane-bool", "label-float", "fill-float", "fill+depth-bool"]


@pytest.mark.parametrize("labels,depth,rules", PLANES, ids=PLANE_IDS)
@pytest.mark.parametrize("size,res,crop", OUTPUTS, ids=[f"{h}x{w}-{c}" for (h, w), _, c in OUTPUTS])
def test_gather_of_put_equals_batch_prep_and_the_cpu_route(size, res, crop, labels, depth, rules, dev, poison):
    H, W = size
    sizes = [(24, 24)] * 3 if (res == 16 and crop is None) else MIXED
    samples = make_samples(sizes, labels=labels, depth=depth, seed=H + W)
    ds = MemorySet(samples, **rules)
    want_depth = depth is not None
    tables = _tables(samples, H, W, res, crop)
    ref, gpu = _caches(ds, 7, H, W, want_depth, dev)
    ref.data.fill_(9)
    gpu.data.fill_(9)
    rows = [6, 0, 3]                                            # a strided subset, the first and the last row in it
    ref.put_tables(rows, samples, tables)
    gpu.put_tables(rows, samples, tables)
    torch.cuda.synchronize()
    assert torch.equal(gpu.data.cpu(), ref.data)                # the named rows' bytes, and every other row untouched
    assert bool((gpu.data[[1, 2, 4, 5]] == 9).all())
    for plane in range(ref.planes if H * W >= 256 else 0):      # the extreme bytes are in every plane (4 x 4 keeps too few pixels to say)
        assert int(ref.data[rows, plane].min()) == 0 or (depth == "plane" and plane == ref.depth_plane)
        assert int(ref.data[rows, plane].max()) == 255
    prep = _batch_prep(ds, samples, tables, H, W, want_depth, dev)
    # n = 1; n = 3 with a repeated index inside a list and one shared between the two; idx_b absent
    for inds, pos in (([3], [6]), ([6, 6, 0], [3, 6, 0]), ([0, 3, 6], None), ([3], None)):
        want = ref.gather(inds, pos)
        got = gpu.gather(inds, pos)
        again = gpu.gather(inds, pos)
        order = torch.tensor([rows.index(i) for i in inds + (pos or [])], device=dev)
        for k, name in enumerate(("img", "label", "mask", "depth")):
            assert same_bits(got[k], want[k]), (name, inds, pos)
            assert same_bits(got[k], again[k]), name
            assert same_bits(got[k], None if prep[k] is None else prep[k][order]), (name, "dg_batch_prep")
        assert got[0].is_cuda and tuple(got[0].shape) == (len(order), 3, H, W)


@pytest.mark.parametrize("rules", [CROPPED, DIRECTORY], ids=["bool", "float"])
def test_null_outputs_one_at_a_time(rules, dev, poison):
    from depthg_amd import ops
    H = W = 20
    samples = make_samples(MIXED, seed=3)
    ds = MemorySet(samples, **rules)
    ref, gpu = _caches(ds, 3, H, W, True, dev)
    for c in (ref, gpu):
        c.put([2, 0, 1], samples, 20, "center")
    full = dict(zip(("img", "label", "mask", "depth"), ref.gather([1, 2], [2, 0])))
    idx = torch.tensor([1, 2, 2, 0], dtype=torch.int64, device=dev)
    for left_out in ("img", "label", "mask", "depth"):
        names = [k for k in full if k != left_out]
        out = ops.sample_cache_gather(gpu.data, True, True, idx[:2], idx[2:], label_offset=ds.label_offset, fill=-1, mask_rule=ds.mask_rule, want=names)
        assert sorted(out) == sorted(names)
        for k in names:
            assert same_bits(out[k], full[k]), (left_out, k)
    only = ops.sample_cache_gather(gpu.data, True, True, idx[:2], None, label_offset=ds.label_offset, mask_rule=ds.mask_rule, want=("mask",))
    assert same_bits(only["mask"], full["mask"][:2])


def test_c_entries_refuse_and_launch_nothing(dev):
    """Every refusal returns an error code with a reason; the cache and the outputs keep their bytes."""
    from depthg_amd import _lib, data, ops
    lib = _lib.load()
    H = W = 8
    samples = make_samples([(12, 10), (9, 14)], seed=1)
    ds = MemorySet(samples, **CROPPED)
    packed, records, table = data.pack_batch(ds, samples, _tables(samples, H, W, 8, "center"), (H, W), True, pin=False)
    cache = torch.full((4, 5, H, W), 7, dtype=torch.uint8, device=dev)
    src = packed.to(dev)
    idx = torch.tensor([1, 3], dtype=torch.int64, device=dev)
    params = torch.cat([records.reshape(-1), table.reshape(-1)]).to(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    def put(cache_t=cache, n_images=4, has_labels=1, with_depth=1, h=H, w=W, idx_t=idx, n=2, src_t=src, nbytes=None, recs=records, tab=table,
            par=params):
        return lib.dg_samplecache_put(p(cache_t), n_images, has_labels, with_depth, h, w, p(idx_t), n, p(src_t),
                                      src.numel() if nbytes is None else nbytes, p(recs), p(tab), p(par), recs.shape[0], stream)

    def changed(col, value, rec=0):
        r = records.clone()
        r[rec, col] = value
        return r
    bad_table = table.clone()
    bad_table[1, 0] = 99
    assert put(n=0) == 0                                                           # nothing to do is not an error
    refused = [put(cache_t=None), put(idx_t=None), put(par=None), put(n_images=0), put(w=6), put(h=0), put(has_labels=2),
               put(cache_t=cache.reshape(-1)[1:]), put(nbytes=src.numel() - 1), put(recs=changed(0, 9)), put(recs=changed(1, 2)),
               put(recs=changed(0, ops.BATCH_LABEL_FILL, rec=1)), put(has_labels=0), put(with_depth=0), put(recs=changed(1, 1)),
               put(recs=records[:-1].contiguous()), put(recs=changed(4, 3)), put(tab=bad_table), put(n=70000)]
    assert all(rc != 0 for rc in refused), refused
    assert b"dg_samplecache_put" in lib.dg_last_error()
    torch.cuda.synchronize()
    assert bool((cache == 7).all())
    assert put() == 0
    torch.cuda.synchronize()
    assert bool((cache[[0, 2]] == 7).all()) and not bool((cache[[1, 3]] == 7).all())

    img = torch.full((4, 3, H, W), 5.0, device=dev)
    label = torch.full((4, H, W), 5, dtype=torch.int64, device=dev)
    mask = torch.zeros((4, H, W), dtype=torch.bool, device=dev)
    depth = torch.full((4, H, W), 5.0, device=dev)
    mean, std = (ctypes.c_float * 3)(*ops.IMAGENET_MEAN), (ctypes.c_float * 3)(*ops.IMAGENET_STD)
    zero_std = (ctypes.c_float * 3)(0.2, 0.0, 0.2)

    def gather(cache_t=cache, n_images=4, has_labels=1, with_depth=1, w=W, a=idx, b=idx, n=2, mean_=mean, std_=std, rule=0, img_t=img, label_t=label,
               mask_t=mask, depth_t=depth):
        return lib.dg_samplecache_gather(p(cache_t), n_images, has_labels, with_depth, H, w, p(a), p(b), n, mean_, std_, -1, -1, rule,
                                         p(img_t), p(label_t), p(mask_t), p(depth_t), stream)
    refused = [gather(cache_t=None), gather(a=None), gather(n_images=0), gather(w=6), gather(with_depth=0), gather(rule=2),
               gather(std_=zero_std), gather(mean_=None), gather(img_t=img.reshape(-1)[1:]), gather(mask_t=mask.reshape(-1)[4:]),
               gather(img_t=None, label_t=None, mask_t=None, depth_t=None), gather(n=40000), gather(cache_t=cache.reshape(-1)[2:])]
    assert all(rc != 0 for rc in refused), refused
    assert b"dg_samplecache_gather" in lib.dg_last_error()
    torch.cuda.synchronize()
    assert bool((img == 5).all()) and bool((label == 5).all()) and not bool(mask.any()) and bool((depth == 5).all())
    assert gather() == 0 and gather(n=0) == 0
    torch.cuda.synchronize()
    assert not bool((img == 5).any()) and not bool((depth[:, 0, 0] == 5).all())
    # the callers check indices on the host; the kernels skip a row outside [0, n_images) all the same
    img.fill_(5.0)
    wild = torch.tensor([4, 1, -1, 3], dtype=torch.int64, device=dev)
    assert gather(a=wild[:2], b=wild[2:], label_t=None, mask_t=None, depth_t=None) == 0
    before = cache.clone()
    assert put(idx_t=torch.tensor([-1, 4], dtype=torch.int64, device=dev)) == 0
    torch.cuda.synchronize()
    assert bool((img[[0, 2]] == 5).all()) and not bool((img[[1, 3]] == 5).any()) and torch.equal(cache, before)


# ---------------------------------------------------------------------------------------------------------------- pipeline, command
def test_contrastive_batches_from_a_sample_cache(tmp_path, dev):
    """The GPU pipeline with a sample cache against the GPU pipeline without one (dg_batch_prep): every key, shape, dtype and bit, with
    no decoding behind the build."""
    from depthg_amd import data
    from depthg_amd.segmenter import default_segmenter_cfg
    root = str(tmp_path)
    sizes = [(37, 23), (23, 37), (64, 64), (50, 20), (30, 25), (64, 64), (23, 37)]
    DF.make_cropped(root, sizes=sizes)
    DF.write_nns(root, "cocostuff27", "train", "five", 16, len(sizes))
    ds = data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train", return_depth=True)
    cfg = default_segmenter_cfg(model_type=DF.MODEL_TYPE, num_neighbors=3, res=16)
    cache = data.build_sample_cache(ds, cfg, 16, "center", True, dev, 2)
    real, loads = ds.load, []
    ds.load = lambda i: (loads.append(i), real(i))[1]
    for pos in (True, False):
        kw = dict(shuffle=pos, pos=pos, device=dev)
        plain = data.ContrastiveBatches(ds, cfg, "train", 16, "center", 3, generator=torch.Generator().manual_seed(5), **kw)
        cached = data.ContrastiveBatches(ds, cfg, "train", 16, "center", 3, generator=torch.Generator().manual_seed(5), sample_cache=cache, **kw)
        torch.manual_seed(4)
        want = list(plain)
        n_plain = len(loads)
        torch.manual_seed(4)
        got = list(cached)
        assert len(loads) == n_plain and len(want) == len(got) == 3
        for a, b in zip(want, got):
            assert list(a) == list(b)
            for k in a:
                assert a[k].device == b[k].device and same_bits(a[k], b[k]), k


SIZES = [(120, 112), (112, 130), (128, 128), (150, 112), (112, 112), (140, 120), (113, 127), (131, 117)]


def test_train_command_with_sample_cache(tmp_path):
    """Three steps of `python -m depthg_amd.train --sample-cache --feature-cache float32` on eight small images: the logged losses equal
    the run without --sample-cache bit for bit (JSON carries a float's repr), and both splits' caches are saved."""
    root = str(tmp_path / "data")
    DF.make_directory(root, sizes=SIZES, split="train", n_classes=5)
    DF.make_directory(root, sizes=SIZES[:4], split="val", n_classes=5, seed=2)
    logs = {}
    for name, extra in (("plain", []), ("cached", ["--sample-cache"])):
        out = str(tmp_path / name)
        args = ["--data-dir", root, "--out", out, "--dataset", "directory", "--precompute-knns", "--feature-cache", "float32"] + extra + \
               ["res=112", "dim=70", "max_steps=3", "val_freq=2", "batch_size=2", "scalar_log_freq=1", "num_workers=2", "crop_type=~",
                "loader_crop_type=center", "num_neighbors=3", "use_depth=False", "depth_feat_correlation_loss=False", "depth_sampling=none",
                "dir_dataset_n_classes=5"]
        run = subprocess.run([sys.executable, "-m", "depthg_amd.train"] + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        assert "3 step(s), 1 validation(s)" in run.stdout
        assert ("sample cache built and saved to" in run.stdout) == bool(extra)
        logs[name] = [json.loads(l) for l in open(os.path.join(out, "log.jsonl"))]
    files = sorted(f for f in os.listdir(root) if f.startswith("sample_cache_"))
    assert len(files) == 2 and "_train_center_112_8_" in files[0] and "_val_center_320_4_" in files[1], files
    steps = {k: [{key: v for key, v in l.items() if key == "step" or key.startswith("loss")} for l in lines if "val" not in l]
             for k, lines in logs.items()}
    assert [l["step"] for l in steps["cached"]] == [1, 2, 3] and all("loss/total" in l for l in steps["cached"])
    assert steps["cached"] == steps["plain"], (steps["cached"], steps["plain"])   # every logged loss of every step
