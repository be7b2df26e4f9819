"""CPU-side checks of the contrastive CRF loss term (dg_crfloss_*, ops.crf_loss_forward / crf_loss_backward,
crf_loss.ContrastiveCRFLoss, cfg.crf_weight in the segmenter): the exports, the refusals before any launch, the compatibility route
against the reference's fixture and the float64 restatement, and the segmenter's configuration keys."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden
import crf_loss_reference as R
from depthg_amd import crf_loss  # noqa: F401  (the module under test: without it nothing here can pass)

NAMES = ["dg_crfloss_workspace_bytes", "dg_crfloss_forward", "dg_crfloss_backward"]


def test_crf_loss_entry_points_are_declared_listed_and_exported():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.fullmatch(r"[a-z_]+", name)
    assert [n for n in _lib.EXPORTS if "crfloss" in n] == NAMES              # the header's order
    assert lib.dg_version() == _lib.DG_VERSION == 119
    assert re.search(r"#define\s+DG_VERSION\s+119\b", header)


def test_workspace_bytes_cover_the_documented_sections():
    from depthg_amd import _lib
    lib = _lib.load()
    for B, D, n in ((2, 5, 1), (2, 70, 257), (32, 70, 1000), (1, 128, 4096)):
        Dp = (D + 3) // 4 * 4
        need = lib.dg_crfloss_workspace_bytes(B, D, n)
        assert need >= B * n * (2 * Dp + 4 + 2) * 4 and need % 256 == 0
    for bad in ((0, 5, 1), (2, 0, 1), (2, 129, 1), (2, 5, 0), (2, 5, 4097)):
        assert lib.dg_crfloss_workspace_bytes(*bad) == 0


def _forward(B=2, D=8, h=4, w=4, H=16, W=16, size=56, n=8, alpha=.5, beta=.15, gamma=.05, ptr=16, code=None, coords=None, ws=None,
             loss=None, ws_bytes=1 << 30):
    """dg_crfloss_forward with dummy addresses: every case here is refused before anything is launched or dereferenced."""
    from depthg_amd import _lib
    lib = _lib.load()
    p = lambda v: ctypes.c_void_p(ptr if v is None else v)
    rc = lib.dg_crfloss_forward(p(code), p(None), B, D, h, w, H, W, size, p(coords), n, alpha, beta, gamma, 10.0, 3.0, 0.0, p(ws), ws_bytes,
                                p(loss), None)
    return rc, lib.dg_last_error().decode()


def _backward(B=2, D=8, h=4, w=4, size=56, n=8, ptr=16, ws=None, coords=None, grad=None, out=None, ws_bytes=1 << 30):
    from depthg_amd import _lib
    lib = _lib.load()
    p = lambda v: ctypes.c_void_p(ptr if v is None else v)
    rc = lib.dg_crfloss_backward(p(ws), ws_bytes, p(coords), B, D, h, w, size, n, p(grad), p(out), None)
    return rc, lib.dg_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_any_launch():
    for call in (_forward, _backward):
        for kw, word in ((dict(D=0), "D="), (dict(D=129), "D="), (dict(n=0), "n="), (dict(n=4097), "n="), (dict(size=0), "size="),
                         (dict(size=257), "size="), (dict(B=0), "positive"), (dict(h=0), "positive"), (dict(w=-1), "positive")):
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (call.__name__, kw, rc, msg)
        rc, msg = call(ptr=0)
        assert rc == -1 and "null" in msg
        rc, msg = call(ws=24)                              # the workspace: 16 bytes
        assert rc == -1 and "aligned" in msg
        rc, msg = call(coords=18)
        assert rc == -1 and "aligned" in msg
        rc, msg = call(ws_bytes=255)
        assert rc == -3 and "workspace" in msg
    for kw in (dict(H=0), dict(W=0)):
        rc, msg = _forward(**kw)
        assert rc == -1 and "positive" in msg, (kw, msg)
    for kw in (dict(alpha=0.0), dict(beta=-1.0), dict(gamma=0.0), dict(alpha=float("nan"))):
        rc, msg = _forward(**kw)
        assert rc == -1 and "alpha=" in msg, (kw, msg)
    for kw in (dict(code=18), dict(loss=6)):
        rc, msg = _forward(**kw)
        assert rc == -1 and "aligned" in msg
    for kw in (dict(grad=18), dict(out=6)):
        rc, msg = _backward(**kw)
        assert rc == -1 and "aligned" in msg


def test_python_routes_refuse_cpu_tensors_and_image_gradients():
    from depthg_amd import ContrastiveCRFLoss, ops
    fn = ContrastiveCRFLoss(8, **R.DEFAULT_SET)
    assert list(fn.parameters()) == []
    img, code = torch.randn(2, 3, 16, 16), torch.randn(2, 5, 4, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        fn.mean_loss(img, code)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.crf_loss_forward(code, img, torch.zeros(2, 8, dtype=torch.int64), 56, .5, .15, .05, 10, 3, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.crf_loss_backward(torch.zeros(1024, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.int64), (2, 5, 4, 4), 56, torch.ones(()))
    with pytest.raises(RuntimeError, match="img"):
        fn.mean_loss(img.clone().requires_grad_(True), code)
    with pytest.raises(ValueError):
        fn(img, code)                                          # maps of different spatial size
    with pytest.raises(ValueError):
        ops.crf_loss_forward(code, img[:, :2], torch.zeros(2, 8, dtype=torch.int64), 56, .5, .15, .05, 10, 3, 0)


@pytest.mark.parametrize("name", ["default", "dense"])
def test_forward_reproduces_the_reference_tensor_and_its_draw(name):
    """torch.manual_seed(seed) and no coords: the two randint calls in the reference's order give the reference's samples."""
    from depthg_amd import ContrastiveCRFLoss
    g = load_golden("crf_loss.npz")
    B, D, h, w = g["clusters"].shape
    assert (B, D, h, w, int(g["n"])) == (2, 6, 9, 7, 32) and g[f"{name}_out"].shape == (2, 32, 32)
    scalars = [float(v) for v in g[f"{name}_scalars"]]
    assert dict(zip(("alpha", "beta", "gamma", "w1", "w2", "shift"), scalars)) == (R.DEFAULT_SET if name == "default" else R.DENSE_SET)
    fn = ContrastiveCRFLoss(int(g["n"]), *scalars)
    torch.manual_seed(int(g["seed"]))
    out = fn(torch.from_numpy(g["guidance"]), torch.from_numpy(g["clusters"]))
    assert out.shape == (2, 32, 32) and out.dtype == torch.float32
    np.testing.assert_allclose(out.numpy(), g[f"{name}_out"], rtol=1e-6, atol=1e-9)
    # the draw itself, and nothing more, is consumed
    torch.manual_seed(int(g["seed"]))
    coords = torch.cat([torch.randint(0, h, size=[1, 32]), torch.randint(0, w, size=[1, 32])], 0)
    after = torch.rand(3)
    torch.manual_seed(int(g["seed"]))
    fn(torch.from_numpy(g["guidance"]), torch.from_numpy(g["clusters"]))
    assert torch.equal(torch.rand(3), after)
    assert torch.equal(fn(torch.from_numpy(g["guidance"]), torch.from_numpy(g["clusters"]), coords=coords), out)


@pytest.mark.parametrize("scalars", [R.DEFAULT_SET, R.DENSE_SET], ids=["default", "dense"])
def test_forward_matches_the_float64_restatement(scalars):
    from depthg_amd import ContrastiveCRFLoss
    gen = torch.Generator().manual_seed(5)
    B, D, s, n = 3, 11, 13, 50
    guidance = torch.randn(B, 3, s, s, generator=gen, dtype=torch.float64)
    clusters = R.normalise(torch.randn(B, D, s, s, generator=gen, dtype=torch.float64))
    coords = torch.stack([torch.randint(0, s, (n,), generator=gen), torch.randint(0, s, (n,), generator=gen)])
    want = R.pair_tensor(guidance, clusters, coords, **scalars)
    fn = ContrastiveCRFLoss(n, **scalars)
    got64 = fn(guidance, clusters, coords=coords)
    assert got64.dtype == torch.float64 and torch.allclose(got64, want, rtol=1e-12, atol=1e-14)
    got32 = fn(guidance.float(), clusters.float(), coords=coords)
    assert torch.allclose(got32.double(), want, rtol=1e-4, atol=2e-5)        # float32 operands: |K| <= 13, |sims| <= 1


def test_restatement_resize_and_norm_are_torch_s():
    """The restatement's own resize and norm against F.interpolate / F.normalize in float64: up- and down-scaling, non-square."""
    gen = torch.Generator().manual_seed(2)
    for h, w, size in ((4, 4, 56), (7, 9, 56), (28, 28, 56), (20, 20, 8), (6, 6, 8), (40, 72, 56), (1, 3, 5)):
        x = torch.randn(2, 3, h, w, generator=gen, dtype=torch.float64)
        want = F.interpolate(x, (size, size), mode="bilinear", align_corners=False)
        assert torch.allclose(R.resize(x, size), want, rtol=1e-12, atol=1e-13), (h, w, size)
    x = torch.randn(2, 5, 3, 3, generator=gen, dtype=torch.float64)
    x[0, :, 1, 1] = 0
    assert torch.allclose(R.normalise(x), F.normalize(x, dim=1, eps=1e-10), rtol=1e-14, atol=0)
    assert torch.equal(R.normalise(x)[0, :, 1, 1], torch.zeros(5, dtype=torch.float64))


def test_segmenter_carries_the_keys_and_builds_the_loss_without_them():
    from depthg_amd import ContrastiveCRFLoss
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    cfg = default_segmenter_cfg()
    want = dict(crf_samples=1000, alpha=.5, beta=.15, gamma=.05, w1=10, w2=3, shift=0)
    for k, v in want.items():
        assert getattr(cfg, k) == v, k
    assert cfg.crf_weight == 0.0
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(res=64, crf_samples=64, alpha=2.0, shift=.25))
    fn = seg.crf_loss_fn
    assert isinstance(fn, ContrastiveCRFLoss) and (fn.n_samples, fn.alpha, fn.beta, fn.gamma, fn.w1, fn.w2, fn.shift) == (64, 2.0, .15, .05, 10, 3, .25)
    bare = default_segmenter_cfg(res=64)
    for k in want:
        delattr(bare, k)
    fn = UnsupervisedSegmenter(5, bare).crf_loss_fn
    assert (fn.n_samples, fn.alpha, fn.beta, fn.gamma, fn.w1, fn.w2, fn.shift) == (1000, .5, .15, .05, 10, 3, 0)
