"""CPU-side checks of the augmentation-alignment term (dg_augalign_*, ops.aug_alignment_forward / aug_alignment_backward,
aug_loss.aug_alignment_loss / crop_flip_coords, cfg.aug_alignment_weight in the segmenter): the exports, the CPU route and the float64
restatement against the reference's fixture, the two transpositions, the coordinate maker, the refusals, and that every GPU test case
has true gradients far above rounding.  (The refusal of GPU tensors that are not float32 needs GPU tensors: tests/test_gpu_aug_alignment.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden
import aug_alignment_reference as R
from depthg_amd import aug_loss  # noqa: F401  (the module under test: without it nothing here can pass)
from depthg_amd.aug_loss import aug_alignment_loss, crop_flip_coords

NAMES = ["dg_augalign_workspace_bytes", "dg_augalign_forward", "dg_augalign_backward"]


def test_entry_points_are_declared_listed_and_exported_under_the_current_version():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [n for n in _lib.EXPORTS if "augalign" in n] == NAMES              # the header's order
    assert lib.dg_version() == _lib.DG_VERSION == 119
    assert re.search(r"#define\s+DG_VERSION\s+119\b", header)


def test_workspace_bytes_and_the_record_bound():
    from depthg_amd import _lib
    lib = _lib.load()
    for B, D, h, w, n in ((2, 5, 4, 4, 3), (32, 70, 28, 28, 28), (2, 70, 56, 56, 56), (1, 1, 1, 1, 1)):
        need = lib.dg_augalign_workspace_bytes(B, D, h, w, n)
        # ds, two norms, s, d u, and the records' offsets, weights and positions
        assert need >= B * n * n * (5 + D) * 4 + B * ((h * w + 1) * 4 + 4 * n * n * 6) and need % 256 == 0
    # 8 h w + 24 n^2 + 4 bytes of LDS, 163776 at most; positions in 16 bits
    assert lib.dg_augalign_workspace_bytes(2, 5, 56, 56, 56) > 0
    assert lib.dg_augalign_workspace_bytes(2, 5, 56, 56, 76) > 0 and lib.dg_augalign_workspace_bytes(2, 5, 56, 56, 77) == 0
    for bad in ((0, 5, 4, 4, 3), (2, 0, 4, 4, 3), (2, 5, 0, 4, 3), (2, 5, 4, -1, 3), (2, 5, 4, 4, 0), (2, 5, 4, 4, 256), (65536, 5, 4, 4, 3),
                (2, 5, 150, 150, 3)):
        assert lib.dg_augalign_workspace_bytes(*bad) == 0, bad


def _forward(B=2, D=8, h=4, w=4, n=4, H=16, W=16, ptr=16, ws_bytes=1 << 30, **at):
    """dg_augalign_forward with dummy addresses: every case here is refused before anything is launched or dereferenced."""
    from depthg_amd import _lib
    lib = _lib.load()
    p = lambda k: ctypes.c_void_p(at.get(k, ptr))
    rc = lib.dg_augalign_forward(p("code"), p("code_aug"), p("coord_aug"), B, D, h, w, n, H, W, p("ws"), ws_bytes, p("loss"), None)
    return rc, lib.dg_last_error().decode()


def _backward(B=2, D=8, h=4, w=4, n=4, ptr=16, ws_bytes=1 << 30, **at):
    from depthg_amd import _lib
    lib = _lib.load()
    p = lambda k: ctypes.c_void_p(at.get(k, ptr))
    rc = lib.dg_augalign_backward(p("code"), p("code_aug"), p("ws"), ws_bytes, B, D, h, w, n, p("grad"), p("d_code"), p("d_code_aug"), None)
    return rc, lib.dg_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_any_launch():
    for call in (_forward, _backward):
        for kw in (dict(B=0), dict(D=0), dict(h=0), dict(w=-1), dict(n=0)):
            rc, msg = call(**kw)
            assert rc == -1 and "positive" in msg, (call.__name__, kw, rc, msg)
        for kw, word in ((dict(n=256), "16 bits"), (dict(h=150, w=150), "LDS"), (dict(h=56, w=56, n=77), "LDS"), (dict(B=65536), "65535")):
            rc, msg = call(**kw)
            assert rc == -2 and word in msg, (call.__name__, kw, rc, msg)
        rc, msg = call(ptr=0)
        assert rc == -1 and "null" in msg
        for kw in (dict(ws=24), dict(code=18), dict(code_aug=6)):
            rc, msg = call(**kw)
            assert rc == -1 and "aligned" in msg, (call.__name__, kw, msg)
        rc, msg = call(ws_bytes=255)
        assert rc == -3 and "workspace" in msg
    for kw in (dict(H=0), dict(W=0)):
        rc, msg = _forward(**kw)
        assert rc == -1 and "positive" in msg
    rc, msg = _forward(H=16385)
    assert rc == -2 and "16384" in msg
    for kw in (dict(coord_aug=18), dict(loss=6)):
        assert _forward(**kw)[0] == -1
    for kw in (dict(grad=18), dict(d_code=6), dict(d_code_aug=10)):
        assert _backward(**kw)[0] == -1


def _fixture(name):
    g = load_golden("aug_alignment.npz")
    return {k[len(name) + 1:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(name + "_")}


@pytest.mark.parametrize("name", ["square", "nonsquare"])
def test_cpu_route_reproduces_the_reference_loss_and_gradients(name):
    g = _fixture(name)
    assert g["code_aug"].shape[2] == g["code_aug"].shape[3] and (name == "square") == (g["code"].shape[2:] == g["code_aug"].shape[2:])
    code, code_aug = g["code"].clone().requires_grad_(True), g["code_aug"].clone().requires_grad_(True)
    loss = aug_alignment_loss(code, code_aug, g["coord_aug"])
    loss.backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32
    # the same torch operations on the same float32 numbers: to float32 rounding
    assert abs(float(loss.detach()) - float(g["loss"])) <= 2 * R.spacing32(float(g["loss"]))
    for got, want in ((code.grad, g["d_code"]), (code_aug.grad, g["d_code_aug"])):
        assert float((got - want).norm() / want.norm()) <= 1e-6


@pytest.mark.parametrize("name", ["square", "nonsquare"])
def test_float64_restatement_reproduces_the_reference(name):
    """The fixture is a float32 computation: its distance from the float64 truth is float32 rounding through the chain - the
    coordinates carry about 1e-7, times the map's side in the taps' weights."""
    g = _fixture(name)
    t = R.chain(g["code"], g["code_aug"], g["coord_aug"])
    assert abs(t["loss"] - float(g["loss"])) <= 1e-6 * t["mean_abs_s"]
    for got, want in ((t["d_code"], g["d_code"]), (t["d_code_aug"], g["d_code_aug"])):
        assert float((got - want.double()).norm() / got.norm()) <= 1e-5
    # and the CPU route in float64 is the restatement to float64 rounding
    code, code_aug = g["code"].double().requires_grad_(True), g["code_aug"].double().requires_grad_(True)
    loss = aug_alignment_loss(code, code_aug, g["coord_aug"].double())
    loss.backward()
    assert abs(float(loss.detach()) - t["loss"]) <= 1e-13
    assert torch.allclose(code.grad, t["d_code"], rtol=1e-9, atol=1e-14) and torch.allclose(code_aug.grad, t["d_code_aug"], rtol=1e-9, atol=1e-14)


def test_restatement_follows_normalize_below_eps():
    """One zero code_aug vector and one zero sampled vector: the restatement's rule is what F.normalize gives under autograd."""
    gen = torch.Generator().manual_seed(4)
    code, code_aug = torch.randn(2, 5, 6, 6, generator=gen, dtype=torch.float64), torch.randn(2, 5, 6, 6, generator=gen, dtype=torch.float64)
    code[0, :, 1:4, 2:5] = 0                                      # the identity grid at n == h == w: u == code up to the float32
    code_aug[1, :, 3, 0] = 0                                      # grid's rounding, so every neighbour of (2, 3) is zero as well
    coord = R.dataset_grid(2, 6, 6).double()
    t = R.chain(code, code_aug, coord)
    assert not bool(t["u"][0, :, 2, 3].any()) and float(t["s"][0, 2, 3]) == 0.0 and float(t["s"][1, 3, 0]) == 0.0
    a, b = code.clone().requires_grad_(True), code_aug.clone().requires_grad_(True)
    R.torch_chain(a, b, coord).backward()
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all())
    assert float(a.grad[0, :, 2, 3].abs().max()) > 1e7 and float(b.grad[1, :, 3, 0].abs().max()) > 1e7       # unit vector / eps / N
    assert torch.allclose(a.grad, t["d_code"], rtol=1e-9, atol=1e-14) and torch.allclose(b.grad, t["d_code_aug"], rtol=1e-9, atol=1e-14)


def test_untransformed_grid_samples_the_map_itself():
    gen = torch.Generator().manual_seed(1)
    code = torch.randn(2, 5, 6, 6, generator=gen)
    # (the dataset's grid at the map's own size: at the image's size the align_corners=False resize of the align_corners=True ramp
    #  does not land on the pixel centres, in the reference as here)
    coord = crop_flip_coords(2, 6, 6, [(0, 0, 6, 6)] * 2, [False, False])
    assert torch.equal(coord, R.dataset_grid(2, 6, 6))
    t = R.chain(code, code, coord)
    assert torch.allclose(t["u"], code.double(), rtol=0, atol=1e-6)
    assert abs(t["loss"] + 1.0) <= 1e-12
    assert abs(float(aug_alignment_loss(code, code, coord)) + 1.0) <= 1e-6
    code_w = torch.randn(2, 5, 7, 9, generator=gen)            # a non-square map on a non-square grid resized to a square one
    t = R.chain(code_w, torch.randn(2, 5, 7, 7, generator=gen), R.dataset_grid(2, 7, 9))
    assert t["u"].shape == (2, 5, 7, 7) and torch.allclose(t["u"][:, :, 3, 3], code_w[:, :, 3, 4].double(), atol=1e-6)


def test_crop_flip_coords():
    full = [(0, 0, 6, 6)] * 2
    flipped = crop_flip_coords(2, 6, 6, full, [True, True])
    grid = R.dataset_grid(2, 6, 6)
    assert torch.equal(flipped[..., 0], grid[..., 0]) and torch.equal(flipped[..., 1], grid[..., 1].flip(2))
    # A flipped full box samples the mirrored map.  With the reference's two transpositions grid_sample reads channel 0 - the ROW
    # coordinate - as x, so the mirrored COLUMN coordinate arrives as y: the mirror is the vertical one.
    gen = torch.Generator().manual_seed(2)
    code = torch.randn(2, 5, 6, 6, generator=gen)
    assert torch.allclose(R.chain(code, code, flipped)["u"], code.flip(2).double(), rtol=0, atol=1e-6)
    ds = F.interpolate(flipped.permute(0, 3, 1, 2), (6, 6), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert torch.allclose(F.grid_sample(code, ds.permute(0, 2, 1, 3), padding_mode="border", align_corners=True), code.flip(2), atol=1e-6)
    # a crop is the bilinear resize (align_corners=False) of the cropped grid
    c = crop_flip_coords(1, 12, 16, [(2, 4, 8, 8)], [False])
    want = F.interpolate(R.dataset_grid(1, 12, 16)[:, 2:10, 4:12].permute(0, 3, 1, 2), (12, 16), mode="bilinear", align_corners=False)
    assert torch.allclose(c, want.permute(0, 2, 3, 1), rtol=0, atol=1e-6)
    assert c.dtype == torch.float32 and float(c.min()) >= -1 and float(c.max()) <= 1
    with pytest.raises(ValueError, match="leaves"):
        crop_flip_coords(1, 12, 16, [(2, 4, 11, 8)], [False])
    with pytest.raises(ValueError, match="boxes"):
        crop_flip_coords(2, 12, 16, [(0, 0, 12, 16)], [False, False])


def test_refusals():
    code, code_aug, coord = torch.randn(2, 5, 4, 4), torch.randn(2, 5, 3, 3), R.dataset_grid(2, 8, 8)
    assert bool(torch.isfinite(aug_alignment_loss(code, code_aug, coord)))
    with pytest.raises(RuntimeError, match="coord_aug"):
        aug_alignment_loss(code, code_aug, coord.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="batch"):
        aug_alignment_loss(code, code_aug[:1], coord)
    with pytest.raises(ValueError, match="batch"):
        aug_alignment_loss(code, code_aug, coord[:1])
    with pytest.raises(ValueError, match=r"\(2, 5, 4, 4\).*\(2, 6, 3, 3\)"):
        aug_alignment_loss(code, torch.randn(2, 6, 3, 3), coord)
    with pytest.raises(ValueError, match="last axis"):
        aug_alignment_loss(code, code_aug, torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError, match=r"square.*\(2, 5, 3, 4\)"):
        aug_alignment_loss(code, torch.randn(2, 5, 3, 4), coord)
    with pytest.raises(ValueError):
        aug_alignment_loss(code[0], code_aug, coord)
    # the ops have no CPU path
    from depthg_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.aug_alignment_forward(code, code_aug, coord)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.aug_alignment_backward(torch.zeros(1024, dtype=torch.uint8), code, code_aug, torch.ones(()))
    with pytest.raises(ValueError, match="square"):
        ops.aug_alignment_forward(code, torch.randn(2, 5, 3, 4), coord)


def test_training_step_names_the_missing_key_before_anything_runs():
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    assert default_segmenter_cfg().aug_alignment_weight == 0.0
    m = UnsupervisedSegmenter(5, default_segmenter_cfg(res=32, aug_alignment_weight=0.5))
    batch = {"img": torch.zeros(2, 3, 32, 32), "img_pos": torch.zeros(2, 3, 32, 32), "label": torch.zeros(2, 32, 32, dtype=torch.long),
             "depth": torch.ones(2, 1, 32, 32), "depth_pos": torch.ones(2, 1, 32, 32), "img_aug": torch.zeros(2, 3, 32, 32)}
    with pytest.raises(KeyError, match="coord_aug"):
        m.training_step(batch, 0)
    del batch["img_aug"]
    batch["coord_aug"] = R.dataset_grid(2, 32, 32)
    with pytest.raises(KeyError, match="img_aug"):
        m.training_step(batch, 0)


@pytest.mark.parametrize("shape,kind", R.CASES)
def test_gpu_cases_have_gradients_far_above_rounding(shape, kind):
    """A relative gradient error means something only where nothing cancels: s away from +-1 (|u^ - s v^|^2 = 1 - s^2), no vector
    near the eps clamp, and both gradients of the size c / |x| predicts."""
    code, code_aug, coord = R.inputs(shape, kind)
    D, (h, w), n, (H, W) = R.SHAPES[shape]
    assert code.shape == (R.B, D, h, w) and code_aug.shape == (R.B, D, n, n) and coord.shape == (R.B, H, W, 2) and coord.dtype == torch.float32
    t = R.truth(shape, kind)
    assert float((1 - t["s"] ** 2).min()) >= 0.02 and float((1 - t["s"] ** 2).mean()) >= 0.3
    assert float(t["u"].square().sum(1).sqrt().min()) >= 0.1 and float(code_aug.square().sum(1).sqrt().min()) >= 0.1
    N = R.B * n * n
    for g in (t["d_code"], t["d_code_aug"]):
        assert float(g.norm()) >= 0.02 / (N ** 0.5 * (D ** 0.5 * 1.2))        # about sqrt(N (1 - s^2)) / (N |x|), |x| ~ 1.2 sqrt(D)
    if kind == "scaled":
        assert float(coord.abs().max()) > 1.2
    if kind == "equal":                                                      # one pixel's list holds every position
        idx, wts = R.taps(R.downsample_coords(coord, n), h, w)
        assert int((idx[0, :, 0] == idx[0, 0, 0]).sum()) == n * n
    if kind == "centres":                                                    # taps of weight exactly zero occur
        idx, wts = R.taps(R.downsample_coords(coord, n), h, w)
        assert int((wts == 0).sum()) >= 3 * 4 * R.B                     # the pinned corners at the least
