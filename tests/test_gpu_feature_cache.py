"""The frozen-backbone feature cache on the GPU: k_fc_put / k_fc_gather (dg_feat_cache.hip) against the class's plain torch route on
the CPU, bit for bit - with one exception, NaN payloads behind a float16 gather: torch's CPU cast widens a float16 NaN among the last
numel % 8 elements of a tensor to 0x7FFFFFFF and every other one by the IEEE rule, so the gather is held to the CPU route's STORED
rows widened exactly (feature_cache_cases.exact_widen) and the CPU route's own output to that everywhere but in its NaNs' payloads;
forward_pair_features against forward_pair; one optimisation step from cached features against the same step
through the backbone; and `python -m depthg_amd.train --feature-cache` on the stub folders."""
import json
import os
import subprocess
import sys

import pytest
import torch

import data_folders as DF
from conftest import ROOT
from feature_cache_cases import exact_widen, feature_rows, same_bits_or_both_nan, special_values

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["float32", "float16", "bfloat16"]
# (C, h, w), N, the rows put, `ind`, `ind_pos`:
#   L = 105: odd, so 16-bit rows start off a 16-byte boundary and fp32 rows off theirs - whole rows element by element, and rows
#            whose head and tail are; three rows
#   L = 128: whole vectors only;  L = 1;  L = 301056 = 384 x 28 x 28 (the training shape: 147 blocks a row) with N = 5, n = 2
#   n = 1 and n = 3, a repeated index inside `ind`, `ind_pos` equal to `ind`
SHAPES = [((3, 5, 7), 7, [6, 0, 3, 2, 5], [0, 6, 3], [5, 2, 0]),
          ((8, 4, 4), 4, [3, 1, 0], [1], [3]),
          ((1, 1, 1), 9, [8, 0, 4, 5, 1, 2, 3], [4, 4, 8], [4, 4, 8]),
          ((6, 1, 2), 5, [4, 1, 2, 3], [2, 2, 4], [1, 3, 3]),            # L = 12: a multiple of 4 and not of 8
          ((384, 28, 28), 5, [4, 1], [1, 4], [4, 4])]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rows():
    """The fp32 rows every kernel case stores, made once per shape."""
    return {shape: feature_rows(len(put), *shape, seed=len(put)) for shape, _, put, _, _ in SHAPES}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,N,put,ind,ind_pos", SHAPES, ids=[f"L{c * h * w}" for (c, h, w), *_ in SHAPES])
def test_kernels_match_the_cpu_route(shape, N, put, ind, ind_pos, dtype, dev, rows):
    from depthg_amd import FeatureCache, ops
    x = rows[shape]
    L = shape[0] * shape[1] * shape[2]
    if L >= special_values().numel():
        assert torch.isnan(x).any() and torch.isinf(x).any()
    ref, gpu = FeatureCache(N, *shape, dtype=dtype, device="cpu"), FeatureCache(N, *shape, dtype=dtype, device=dev)
    sentinel = torch.full((N, L), 3.0, dtype=dtype)              # a put leaves every other row alone, row 0 and the last row included
    ref.data.copy_(sentinel)
    gpu.data.copy_(sentinel)
    ref.put(put, x)
    gpu.put(put, x.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(gpu.data.cpu().view(torch.int16 if dtype != torch.float32 else torch.int32),
                       ref.data.view(torch.int16 if dtype != torch.float32 else torch.int32))
    assert gpu.filled.tolist() == ref.filled.tolist()
    # one list, and two lists in one launch: views of one allocation.  The reference is the CPU route's stored rows widened exactly
    # (exact_widen: torch's own cast, but for the NaNs its CPU float16 cast widens by position in the tensor); the CPU route's own
    # output agrees with it wherever it holds no NaN.
    def rows_of(idx):
        return exact_widen(ref.data.index_select(0, torch.tensor(idx))).reshape((len(idx),) + shape)

    want = rows_of(ind)
    assert same_bits_or_both_nan(ref.gather(ind), want)
    got = gpu.gather(ind)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(ind),) + shape
    assert torch.equal(_bits(got.cpu()), _bits(want))
    wa, wb = rows_of(ind), rows_of(ind_pos)
    ca, cb = ref.gather(ind, ind_pos)
    assert same_bits_or_both_nan(ca, wa) and same_bits_or_both_nan(cb, wb)
    ga, gb = gpu.gather(ind, ind_pos)
    assert gb.data_ptr() == ga.data_ptr() + ga.numel() * 4
    assert torch.equal(_bits(ga.cpu()), _bits(wa)) and torch.equal(_bits(gb.cpu()), _bits(wb))
    if dtype != torch.float32:
        assert torch.equal(_bits(wa), _bits(exact_widen(x[[put.index(i) for i in ind]].to(dtype))))
    # every element of a poisoned output is overwritten (0xFF bytes: what DG_POISON fills buffers with)
    n = len(ind)
    idx = torch.tensor(ind + ind_pos, dtype=torch.int64, device=dev)
    out = torch.empty(2 * n, L, dtype=torch.float32, device=dev)
    out.view(torch.uint8).fill_(0xFF)
    ops.feature_cache_gather(gpu.data, idx[:n], idx[n:], out=out)
    assert torch.equal(_bits(out.cpu()), _bits(torch.cat([wa, wb]).reshape(2 * n, L)))
    out1 = torch.empty(n, L, dtype=torch.float32, device=dev)
    out1.view(torch.uint8).fill_(0xFF)
    ops.feature_cache_gather(gpu.data, idx[:n], None, out=out1)
    assert torch.equal(_bits(out1.cpu()), _bits(wa.reshape(n, L)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_put_to_the_last_row_leaves_row_zero(dtype, dev):
    from depthg_amd import FeatureCache
    shape, N = (3, 5, 7), 4
    x = feature_rows(2, *shape, seed=9)
    gpu = FeatureCache(N, *shape, dtype=dtype, device=dev)
    gpu.put([0], x[:1].to(dev))
    before = gpu.data.cpu().clone()
    gpu.put([N - 1], x[1:].to(dev))
    after = gpu.data.cpu()
    view = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(after[:N - 1].view(view), before[:N - 1].view(view))              # rows 0 .. N - 2 untouched, bit for bit
    assert torch.equal(_bits(gpu.gather([0]).cpu()), _bits(exact_widen(x[:1].to(dtype))))
    assert torch.equal(_bits(gpu.gather([N - 1]).cpu()), _bits(exact_widen(x[1:].to(dtype))))


def test_unaligned_tensors_and_refusals(dev):
    """Rows that meet a 16-byte boundary only behind a head (the cache and the output one element into their buffers), and what
    ops refuses before a launch."""
    from depthg_amd import ops
    N, L, n = 3, 37, 2
    x = feature_rows(N, 1, 1, L, seed=4).reshape(N, L)
    for dtype in DTYPES:
        for off_c, off_o in ((1, 1), (2, 0), (4, 4), (3, 2), (0, 3)):
            buf = torch.zeros(N * L + 8, dtype=dtype, device=dev)
            cache = buf[off_c:off_c + N * L].view(N, L)
            idx = torch.tensor([2, 0, 1], dtype=torch.int64, device=dev)
            ops.feature_cache_put(cache, idx, x.to(dev))
            want = torch.zeros(N, L, dtype=dtype)
            want[[2, 0, 1]] = x.to(dtype)
            assert torch.equal(_bits(exact_widen(cache.cpu())), _bits(exact_widen(want))), (dtype, off_c)
            assert float(buf[:off_c].float().abs().sum()) == 0 and float(buf[off_c + N * L:].float().abs().sum()) == 0
            obuf = torch.zeros(2 * n * L + 8, dtype=torch.float32, device=dev)
            out = obuf[off_o:off_o + 2 * n * L].view(2 * n, L)
            out.fill_(float("nan"))
            ops.feature_cache_gather(cache, idx[:n], idx[1:], out=out)
            assert torch.equal(_bits(out.cpu()), _bits(exact_widen(want[[2, 0, 0, 1]]))), (dtype, off_c, off_o)
            assert float(obuf[:off_o].abs().sum()) == 0 and float(obuf[off_o + 2 * n * L:].abs().sum()) == 0
    cache = torch.zeros(N, L, dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match="int64"):
        ops.feature_cache_gather(cache, torch.tensor([0], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="on cuda"):
        ops.feature_cache_gather(cache, torch.tensor([0], dtype=torch.int64))
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        ops.feature_cache_gather(cache.double(), torch.tensor([0], dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="rows of"):
        ops.feature_cache_put(cache, torch.tensor([0], dtype=torch.int64, device=dev), torch.zeros(2, L, device=dev))
    # the host checks indices first (FeatureCache); the kernels skip a row index outside [0, N) all the same.  The cache is the
    # middle of a larger zeroed buffer here, whose rows in front of it and behind it stay zero.
    big = torch.zeros(N + 2, L, dtype=torch.float16, device=dev)
    cache = big[1:N + 1]
    ops.feature_cache_put(cache, torch.tensor([-1, 2, N], dtype=torch.int64, device=dev), torch.ones(3, L, device=dev))
    assert float(big[0].abs().max()) == 0.0 and float(big[N + 1].abs().max()) == 0.0
    big[0].fill_(7.0)
    big[N + 1].fill_(7.0)
    out = torch.full((3, L), 5.0, device=dev)
    ops.feature_cache_gather(cache, torch.tensor([N, 2, -1], dtype=torch.int64, device=dev), None, out=out)
    torch.cuda.synchronize()
    assert float(cache[:2].abs().max()) == 0.0 and float(cache[2].min()) == 1.0
    assert float(out[0].min()) == 5.0 and float(out[2].min()) == 5.0 and float(out[1].min()) == 1.0 and float(out[1].max()) == 1.0


# ---------------------------------------------------------------------------------------------------------------- featurizer, step
def _cfg(kind, **over):
    from depthg_amd.segmenter import default_segmenter_cfg
    if kind == "dino":          # a two-block ViT (head dimension 64), 40 x 40 images: a 5 x 5 feature grid
        base = dict(model_type="vit_small", dino_patch_size=8, dg_dino_backbone=True, feature_samples=5,
                    dg_dino_vit_kwargs=dict(img_size=[32], embed_dim=128, depth=2, num_heads=2))
    elif kind == "standin40":   # the stand-in backbone at 40 x 40: the same 5 x 5 grid, 384 channels
        base = dict(dim=70, feature_samples=5)
    else:                       # the stand-in backbone at 112 x 112: a 14 x 14 grid of 384 channels, 11 x 11 samples (the default recipe)
        base = dict(dim=70, feature_samples=11)
    return default_segmenter_cfg(**{**base, **over})


def _batch(kind, dev, B=4, n_classes=5, seed=0):
    hw = 112 if kind == "standin" else 40
    g = torch.Generator().manual_seed(seed)
    return {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
            "label": torch.randint(0, n_classes, (B, hw, hw), generator=g).to(dev),
            "depth": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev),
            "depth_pos": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev)}


def _segmenter(kind, dev, **over):
    import warnings
    from depthg_amd.segmenter import UnsupervisedSegmenter
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)            # (the ViT keeps its seeded random weights)
        seg = UnsupervisedSegmenter(5, _cfg(kind, **over)).to(dev)
    seg.train()
    return seg


@pytest.mark.parametrize("kind", ["standin", "dino"])
@pytest.mark.parametrize("defer", [False, True], ids=["applied", "deferred"])
def test_forward_pair_features_equals_forward_pair(kind, defer, dev):
    from depthg_amd.ops import DeferredDropout
    net = _segmenter(kind, dev).net
    batch = _batch(kind, dev)
    with torch.no_grad():
        f, fp = net._backbone(batch["img"])[0], net._backbone(batch["img_pos"])[0]
    torch.manual_seed(5)
    want = net.forward_pair(batch["img"], batch["img_pos"], defer)
    torch.manual_seed(5)
    got = net.forward_pair_features(f, fp, defer)

    def flat(passes):
        out = []
        for feats, code, _ in passes:
            if isinstance(feats, DeferredDropout):
                assert defer
                out += [v for v in vars(feats).values() if isinstance(v, torch.Tensor)]
            else:
                out.append(feats)
            out.append(code)
        return out

    a, b = flat(want), flat(got)
    assert len(a) == len(b) and len(a) >= 4
    for u, v in zip(a, b):
        assert u.shape == v.shape and torch.equal(_bits(u.float()), _bits(v.float()))
    assert got[0][2] is None and got[1][2] is None
    # one pass: forward_features against forward
    torch.manual_seed(6)
    w1 = net(batch["img"])
    torch.manual_seed(6)
    g1 = net.forward_features(f)
    assert torch.equal(_bits(w1[0]), _bits(g1[0])) and torch.equal(_bits(w1[1]), _bits(g1[1])) and g1[2] is None


def _step(kind, dev, batch, monkeypatch, over, cache_dtype=None):
    """One training_step of a freshly seeded segmenter on `batch`; with `cache_dtype` the batch carries image_feat / image_feat_pos
    gathered from a FeatureCache filled from the backbone on the same tensors.  -> (loss, logs, gradients of the stepped parameters,
    the feature maps that entered the head)."""
    from depthg_amd import FeatureCache, featurizer
    # (torch's own convolutions - the stand-in backbone, the linear probe and its backward - with deterministic algorithms, for the
    #  cache's fill as for the step)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    seg = _segmenter(kind, dev, dg_feature_cache=None if cache_dtype is None else str(cache_dtype).replace("torch.", ""), **over)
    if cache_dtype is not None:
        B = batch["img"].shape[0]
        with torch.no_grad():
            f, fp = seg.net._backbone(batch["img"])[0], seg.net._backbone(batch["img_pos"])[0]
        cache = FeatureCache(2 * B + 1, *f.shape[1:], dtype=cache_dtype, device=dev)
        cache.put(list(range(B)), f)
        cache.put(list(range(B + 1, 2 * B + 1)), fp)
        batch = dict(batch)
        batch["image_feat"], batch["image_feat_pos"] = cache.gather(list(range(B)), list(range(B + 1, 2 * B + 1)))
        monkeypatch.setattr(seg.net, "_backbone", lambda *a, **k: pytest.fail("the cached step ran the backbone"))
    entered = []
    for name in ("run_head", "run_head_pair"):
        real = getattr(featurizer, name)

        def spy(c1, c2, *rest, _real=real, _n=(1 if name == "run_head" else 2)):
            entered.extend(t.detach().clone() for t in rest[:_n])
            return _real(c1, c2, *rest)
        monkeypatch.setattr(featurizer, name, spy)
    grads = []
    torch.manual_seed(7)
    loss, logs = seg.training_step(batch, 0, grad_sync=lambda: grads.extend(p.grad.detach().clone() for p in seg.all_reduced_parameters()))
    torch.cuda.synchronize()
    monkeypatch.undo()
    return loss, logs, grads, entered


def _same_bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


# Every case runs the uncached step twice first and measures, per gradient, what that pair's own difference is.  On the 5 x 5 grid the
# step is required to repeat itself bit for bit, and the cached step is held to the same bits.  At 112 x 112 (a 14 x 14 grid, the
# default recipe's 11 x 11 samples) the linear probe's weight gradient - torch's convolution backward - was seen to differ between two
# uncached runs in its last bit (7e-10 - 9e-10) unless torch is asked for deterministic convolution algorithms, which _step does; the
# case asserts no premise and applies the rule to whatever the pair measures: a gradient the pair repeats must come out of the cached
# step with the same bits, one it does not repeat may differ from the uncached step by no more than the pair's own difference.
STEP_CASES = [("standin40", {}, True),                                       # paired
              ("standin40", {"lhp": True}, True),                            # unpaired: the LHP module stands between the passes
              ("dino", {}, True), ("dino", {"lhp": True}, True),             # the two-block ViT, paired and unpaired
              ("standin", {}, False)]                                        # the default recipe at 112 x 112
STEP_IDS = ["standin-paired", "standin-unpaired", "dino-paired", "dino-unpaired", "standin-112"]


@pytest.mark.parametrize("kind,over,must_repeat", STEP_CASES, ids=STEP_IDS)
def test_step_from_a_float32_cache_equals_the_step_through_the_backbone(kind, over, must_repeat, dev, monkeypatch):
    """The premise first: the uncached step, run twice from the same seeds, gives the same bits - its forward always, its gradients
    where `must_repeat`.  Then the cached step against it: the features entering the head, the loss and every log scalar bit for
    bit; every stepped parameter's gradient bit for bit where the uncached pair's own is, else within the pair's own difference."""
    batch = _batch(kind, dev)
    l0, logs0, g0, e0 = _step(kind, dev, batch, monkeypatch, over)
    l1, logs1, g1, e1 = _step(kind, dev, batch, monkeypatch, over)
    assert len(e0) == 2 and len(g0) >= 6 and len(g0) == len(g1)
    assert all(_same_bits(a, b) for a, b in zip(e0, e1))
    assert _same_bits(l0, l1) and set(logs0) == set(logs1) and all(_same_bits(logs0[k], logs1[k]) for k in logs0), \
        "the uncached step's forward does not repeat itself on this machine"
    pair = [float((a - b).abs().max()) for a, b in zip(g0, g1)]
    repeated = [_same_bits(a, b) for a, b in zip(g0, g1)]
    if must_repeat:
        assert all(repeated), f"the uncached step's gradients do not repeat themselves on this machine: {pair}"
    lc, logsc, gc, ec = _step(kind, dev, batch, monkeypatch, over, cache_dtype=torch.float32)
    assert len(ec) == 2
    for a, b in zip(e0, ec):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), "the features entering the head differ"
    print(f"{kind} {over}: loss uncached {float(l0)!r} cached {float(lc)!r}")
    assert _same_bits(l0, lc)
    assert set(logs0) == set(logsc)
    for k in logs0:
        assert _same_bits(logs0[k], logsc[k]), k
    assert len(g0) == len(gc)
    cached = [float((a - b).abs().max()) for a, b in zip(g0, gc)]
    print(f"{kind} {over}: max |d gradient| uncached vs uncached {pair}, cached vs uncached {cached}")
    for i, (a, b) in enumerate(zip(g0, gc)):
        assert a.shape == b.shape and bool(torch.isfinite(b).all())
        if repeated[i]:
            assert _same_bits(a, b), f"gradient {i}"
        else:
            assert cached[i] <= pair[i], f"gradient {i}: cached vs uncached {cached[i]} above the uncached pair's own {pair[i]}"


def test_step_from_a_float16_cache(dev, monkeypatch):
    """The features entering the head are image_feat.half().float(); the step runs and is finite.  The distance of its loss from the
    float32 step's is printed, not bounded: nobody has measured it on real DINO weights."""
    kind, over = "standin", {}
    batch = _batch(kind, dev)
    l32, _, _, e32 = _step(kind, dev, batch, monkeypatch, over)
    l16, logs16, g16, e16 = _step(kind, dev, batch, monkeypatch, over, cache_dtype=torch.float16)
    for a, b in zip(e32, e16):
        assert torch.equal(_bits(a.half().float()), _bits(b))
    assert bool(torch.isfinite(l16)) and all(bool(torch.isfinite(g).all()) for g in g16)
    assert all(bool(torch.isfinite(torch.as_tensor(v).float()).all()) for v in logs16.values())
    print(f"float16 cache: loss {float(l16)!r}, float32 {float(l32)!r}, difference {float(l16) - float(l32):.3e}")


def test_step_ignores_the_keys_without_the_cfg_key(dev, monkeypatch):
    """cfg.dg_feature_cache absent: a batch that carries the two keys still goes through the backbone."""
    kind = "standin"
    batch = _batch(kind, dev)
    l0, _, _, e0 = _step(kind, dev, batch, monkeypatch, {})
    poisoned = {**batch, "image_feat": torch.full_like(e0[0], float("nan")), "image_feat_pos": torch.full_like(e0[1], float("nan"))}
    l1, _, _, e1 = _step(kind, dev, poisoned, monkeypatch, {})
    assert _same_bits(l0, l1) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(e0, e1))


# ---------------------------------------------------------------------------------------------------------------- train command
SIZES = [(120, 112), (112, 130), (128, 128), (150, 112), (112, 112), (140, 120), (113, 127), (131, 117)]


def test_train_command_with_feature_cache(tmp_path):
    """Three steps of `python -m depthg_amd.train --feature-cache float32` on eight small images (the shapes of
    tests/test_gpu_train_loop.py, with the centre crop a cache needs); a second invocation loads the saved cache instead of building it."""
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    DF.make_directory(root, sizes=SIZES, split="train", n_classes=5)
    DF.make_directory(root, sizes=SIZES[:4], split="val", n_classes=5, seed=2)
    args = ["--data-dir", root, "--out", out, "--dataset", "directory", "--precompute-knns", "--feature-cache", "float32", "res=112", "dim=70",
            "max_steps=3", "val_freq=2", "batch_size=2", "scalar_log_freq=1", "num_workers=2", "crop_type=~", "loader_crop_type=center",
            "num_neighbors=3", "use_depth=False", "depth_feat_correlation_loss=False", "depth_sampling=none", "dir_dataset_n_classes=5"]
    run = subprocess.run([sys.executable, "-m", "depthg_amd.train"] + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "3 step(s), 1 validation(s)" in run.stdout and "feature cache built and saved to" in run.stdout
    files = [f for f in os.listdir(root) if f.startswith("feature_cache_") and f.endswith("_float32.pt")]
    assert len(files) == 1, os.listdir(root)
    path = os.path.join(root, files[0])
    assert os.path.getsize(path) > 8 * 384 * 14 * 14 * 4
    mtime = os.stat(path).st_mtime_ns
    lines = [json.loads(l) for l in open(os.path.join(out, "log.jsonl"))]
    steps = [l for l in lines if "val" not in l]
    assert [l["step"] for l in steps] == [1, 2, 3]
    for l in steps:
        assert l["loss/total"] == l["loss/total"] and abs(l["loss/total"]) < float("inf")
    out2 = str(tmp_path / "out2")
    run2 = subprocess.run([sys.executable, "-m", "depthg_amd.train"] + [out2 if a == out else a for a in args], cwd=ROOT, capture_output=True,
                          text=True, timeout=240)
    assert run2.returncode == 0, run2.stdout[-2000:] + run2.stderr[-4000:]
    assert "feature cache loaded from" in run2.stdout and "feature cache built" not in run2.stdout
    assert os.stat(path).st_mtime_ns == mtime
    steps2 = [l for l in (json.loads(l) for l in open(os.path.join(out2, "log.jsonl"))) if "val" not in l]
    assert [l["step"] for l in steps2] == [1, 2, 3]
