"""CPU-side checks of the GPU batch augmentation (dg_augment_*, ops.augment_forward, augment.draw_augment_params / augment_batch,
cfg.dg_gpu_augment in the segmenter): the exports, the float64 restatement against torch's own resize and against its own properties,
the parameter draws, the CPU route against the restatement and against crop_flip_coords, the segmenter's key, the refusals."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
import augment_reference as R
from depthg_amd import augment as A
from depthg_amd.aug_loss import crop_flip_coords

NAMES = ["dg_augment_workspace_bytes", "dg_augment_forward"]
EPS32 = 2.0 ** -24


def _params(B, H, W, **over):
    p = A.identity_params(B, H, W)._asdict()
    for k, v in over.items():
        p[k] = torch.as_tensor(v, dtype=p[k].dtype).reshape(p[k].shape)
    return A.AugmentParams(**p)


def test_entry_points_are_declared_listed_and_exported_under_the_current_version():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [n for n in _lib.EXPORTS if n.startswith("dg_augment_")] == NAMES              # the header's order
    assert lib.dg_version() == _lib.DG_VERSION == 119
    assert _lib.SIGNATURES["dg_augment_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int32] * 3)
    assert len(_lib.SIGNATURES["dg_augment_forward"][1]) == 20
    # one fp64 partial per statistics block, at most 64 per image
    assert lib.dg_augment_workspace_bytes(32, 224, 224) == 32 * 56 * 8 and lib.dg_augment_workspace_bytes(2, 1024, 1024) == 2 * 64 * 8
    assert lib.dg_augment_workspace_bytes(1, 5, 5) == 256
    for bad in ((0, 8, 8), (65536, 8, 8), (2, 2, 8), (2, 8, 2), (2, 16385, 8)):
        assert lib.dg_augment_workspace_bytes(*bad) == 0, bad


@pytest.mark.parametrize("flip,box,out", [(False, (0, 0, 9, 11), (9, 11)), (True, (1, 2, 7, 8), (9, 11)), (True, (0, 3, 8, 8), (12, 17)),
                                          (False, (2, 0, 7, 11), (7, 11))])
def test_restatement_resample_is_torch_bilinear(flip, box, out):
    x = torch.rand(3, 9, 11, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    top, left, bh, bw = box
    crop = (x.flip(-1) if flip else x)[:, top:top + bh, left:left + bw]
    want = F.interpolate(crop[None].double(), out, mode="bilinear", align_corners=False)[0]
    got = torch.from_numpy(R.resample(x.numpy(), flip, box, out))
    assert float((got - want).abs().max()) <= 1e-12


def test_restatement_properties():
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, (3, 7, 9))
    for sigma in (0.1, 0.7, 2.0):
        assert abs(R.blur_kernel(sigma).sum() - 1.0) <= 1e-15
        const = np.full((3, 7, 9), 0.37)
        assert np.abs(R.blur(const, sigma) - const).max() <= 1e-15
    assert np.abs(R.contrast(x, 1.0) - x).max() <= 1e-15 and np.abs(R.saturation(x, 1.0) - x).max() <= 1e-15
    sat = rng.uniform(0.05, 0.95, (3, 7, 9))
    sat[rng.integers(0, 3, (7, 9)), np.arange(7)[:, None], np.arange(9)[None]] *= 0.3       # no channel ties: a saturated image
    for f in (0.07, -0.1, 0.31):
        assert np.abs(R.hue(R.hue(sat, f), -f) - sat).max() <= 1e-12
    g = np.repeat(rng.uniform(0.0, 1.0, (1, 7, 9)), 3, 0)
    unit = sum(R.GRAY)                                         # 0.9999: the gray of a gray image is 0.9999 of it
    assert np.abs(R.gray(g) - unit * g[0]).max() <= 1e-15
    assert np.abs(R.saturation(g, 1.0) - g).max() <= 1e-15
    assert np.abs(R.saturation(g, 0.6) - (0.6 + 0.4 * unit) * g).max() <= 1e-15
    assert np.abs(R.hue(g, 0.2) - g).max() <= 1e-15          # s = 0: hue moves nothing


def test_draws_are_seeded_in_range_and_cover_every_order():
    a = A.draw_augment_params(16, 224, 224, torch.Generator().manual_seed(11))
    b = A.draw_augment_params(16, 224, 224, torch.Generator().manual_seed(11))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert [t.dtype for t in a] == [torch.bool, torch.int32, torch.int8, torch.float32, torch.bool, torch.float32]
    assert [tuple(t.shape) for t in a] == [(16,), (16, 4), (16, 4), (16, 4), (16,), (16,)]
    p = A.draw_augment_params(2000, 224, 224, torch.Generator().manual_seed(12))
    top, left, bh, bw = (p.box[:, k].long() for k in range(4))
    assert bool(((top >= 0) & (left >= 0) & (bh > 0) & (bw > 0) & (top + bh <= 224) & (left + bw <= 224)).all())
    # w = round(sqrt(area * aspect)), h = round(sqrt(area / aspect)): each side moves by at most half a pixel
    frac = (bh * bw).double() / 224 ** 2
    slack = 0.5 * (bh + bw).double() / 224 ** 2 + 0.25 / 224 ** 2
    assert bool((frac >= 0.8 - slack).all()) and bool((frac <= 1.0 + slack).all())
    f = p.factors
    for k in range(3):
        assert 0.7 <= float(f[:, k].min()) and float(f[:, k].max()) <= 1.3
    assert -0.1 <= float(f[:, 3].min()) and float(f[:, 3].max()) <= 0.1
    assert 0.6 < float(f[:, 0].min()) + float(f[:, 0].max()) - 1.0 < 1.4 and float(f[:, 0].std()) > 0.1       # spread over the range
    assert {tuple(o) for o in p.ops.tolist()} == set(itertools.permutations(range(4)))
    assert 0.4 < float(p.flip.float().mean()) < 0.6 and 0.15 < float(p.gray.float().mean()) < 0.25
    blurred = p.blur_sigma > 0
    assert 0.4 < float(blurred.float().mean()) < 0.6
    assert 0.1 <= float(p.blur_sigma[blurred].min()) and float(p.blur_sigma[blurred].max()) <= 2.0
    # the global generator is the default
    torch.manual_seed(5)
    c = A.draw_augment_params(3, 32, 32)
    torch.manual_seed(5)
    d = A.draw_augment_params(3, 32, 32)
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    doc = A.draw_augment_params.__doc__
    assert "randperm(4)" in doc and "NOT claimed" in doc


def _mixed_case(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g) * 0.96 + 0.02
    return img, A.draw_augment_params(B, H, W, g, p_blur=0.7, p_gray=0.3)


@pytest.mark.parametrize("out_size,unit", [(None, False), ((13, 30), False), (None, True)])
def test_cpu_route_equals_the_restatement_within_float32_rounding(out_size, unit):
    img, p = _mixed_case(21, 6, 19, 23)
    kw = dict(mean=A.IMAGENET_MEAN, std=A.IMAGENET_STD) if unit else {}
    if unit:
        img = (img - torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1)
    got, _ = A.augment_batch(img, p, out_size=out_size, **kw)
    truth = R.augment(img, p, out_size, **kw)
    max_abs, rel = R.errors(got, truth)
    # the chain is at most ~40 float32 roundings deep on values of size <= 1 (<= 1 / min std = 4.5 in the normalised space), hue's
    # divisions amplify by 1 / (max - min) of a pixel, bounded through the inputs' spread: a generous 2e-4 catches every formula error
    # (those are >= 1e-3) and no rounding
    assert float(max_abs.max()) <= 2e-4 * (4.5 if unit else 1.0), max_abs
    assert float(rel.max()) <= 2e-5, rel
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(truth.shape)


def test_cpu_route_coord_aug_is_crop_flip_coords_bit_for_bit():
    img, p = _mixed_case(22, 5, 17, 29)
    _, coord = A.augment_batch(img, p)
    want = crop_flip_coords(5, 17, 29, [tuple(b) for b in p.box.tolist()], p.flip.tolist())
    assert coord.dtype == torch.float32 and torch.equal(coord, want)


def test_identity_record_returns_the_image_and_the_grid_bit_for_bit():
    img = torch.randn(3, 3, 9, 14, generator=torch.Generator().manual_seed(2))
    got, coord = A.augment_batch(img, A.identity_params(3, 9, 14))
    assert torch.equal(got, img) and torch.equal(coord, R.dataset_grid(3, 9, 14))


class _TinyNet(torch.nn.Module):
    """A CPU stand-in featurizer: (feats, code, attn) of a 4 x 4 patch convolution."""
    def __init__(self, dim):
        super().__init__()
        self.n_feats = 8
        self.conv = torch.nn.Conv2d(3, dim, 4, stride=4)

    def forward(self, img):
        code = self.conv(img)
        return code.detach(), code, None


class _TinyProbe(torch.nn.Module):
    """A CPU stand-in for the cluster probe (ClusterLookup's loss is a HIP kernel): (loss, None)."""
    def __init__(self, dim):
        super().__init__()
        self.clusters = torch.nn.Parameter(torch.ones(dim))

    def forward(self, code, _):
        return (code * self.clusters.view(1, -1, 1, 1)).square().mean(), None


def _cpu_step(monkeypatch, **cfg_over):
    """An UnsupervisedSegmenter whose step runs on the CPU: the correlation term off, the featurizer and the two probe losses (HIP
    only) replaced by torch stand-ins; the augmentation-alignment term and the augmentation have CPU routes of their own."""
    from depthg_amd import segmenter as S
    cfg = S.default_segmenter_cfg(res=16, aug_alignment_weight=0.5, correspondence_weight=0.0, **cfg_over)
    dim = cfg.dim if cfg.continuous else 5
    m = S.UnsupervisedSegmenter(5, cfg, net=_TinyNet(dim))
    monkeypatch.setattr(S, "probe_cross_entropy", lambda logits, label: logits.square().mean())
    m.cluster_probe = _TinyProbe(dim)
    g = torch.Generator().manual_seed(9)
    batch = {"img": torch.rand(2, 3, 16, 16, generator=g), "img_pos": torch.rand(2, 3, 16, 16, generator=g),
             "label": torch.zeros(2, 16, 16, dtype=torch.long), "depth": torch.ones(2, 1, 16, 16), "depth_pos": torch.ones(2, 1, 16, 16)}
    return m, batch


def test_segmenter_key_off_keeps_the_key_error(monkeypatch):
    m, batch = _cpu_step(monkeypatch)
    assert not getattr(m.cfg, "dg_gpu_augment", False)
    state = torch.get_rng_state()
    with pytest.raises(KeyError, match="img_aug"):
        m.training_step(batch, 0)
    assert torch.equal(torch.get_rng_state(), state)


def test_segmenter_key_on_augments_logs_and_draws(monkeypatch):
    m, batch = _cpu_step(monkeypatch, dg_gpu_augment=True)
    keys = set(batch)
    weights = {k: v.clone() for k, v in m.state_dict().items()}      # (the step moves them)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    loss, logs = m.training_step(batch, 0)
    assert "loss/aug_alignment" in logs and bool(torch.isfinite(logs["loss/aug_alignment"])) and bool(torch.isfinite(loss))
    assert not torch.equal(torch.get_rng_state(), state)          # the parameters came from the global generator
    assert set(batch) == keys                                     # the caller's batch is not written to
    # the step's term is the term of augment_batch's tensors for the same seeded parameters
    torch.manual_seed(3)
    p = A.draw_augment_params(2, 16, 16)
    img_aug, coord_aug = A.augment_batch(batch["img"], p)
    m2, _ = _cpu_step(monkeypatch)
    m2.load_state_dict(weights)
    _, logs2 = m2.training_step({**batch, "img_aug": img_aug, "coord_aug": coord_aug}, 0)
    assert torch.equal(logs2["loss/aug_alignment"], logs["loss/aug_alignment"])
    # a batch that carries the keys wins, untouched: nothing is drawn
    m3, _ = _cpu_step(monkeypatch, dg_gpu_augment=True)
    m3.load_state_dict(weights)
    state = torch.get_rng_state()
    _, logs3 = m3.training_step({**batch, "img_aug": img_aug, "coord_aug": coord_aug}, 0)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(logs3["loss/aug_alignment"], logs["loss/aug_alignment"])
    # "unit": the colour ops see de-normalised values - another img_aug, hence another term
    m4, _ = _cpu_step(monkeypatch, dg_gpu_augment="unit")
    m4.load_state_dict(weights)
    torch.manual_seed(3)
    _, logs4 = m4.training_step(batch, 0)
    assert bool(torch.isfinite(logs4["loss/aug_alignment"])) and not torch.equal(logs4["loss/aug_alignment"], logs["loss/aug_alignment"])


def test_segmenter_weight_zero_draws_nothing(monkeypatch):
    m, batch = _cpu_step(monkeypatch, dg_gpu_augment=True)
    m.cfg.aug_alignment_weight = 0.0
    state = torch.get_rng_state()
    _, logs = m.training_step(batch, 0)
    assert torch.equal(torch.get_rng_state(), state) and "loss/aug_alignment" not in logs


def _forward(B=2, C=3, H=16, W=16, h=16, w=16, ptr=16, ws_bytes=1 << 20, strides=None, recs=None, mean=None, std=None, **at):
    """dg_augment_forward with dummy addresses: every case here is refused before anything is launched or dereferenced on the device."""
    from depthg_amd import _lib
    lib = _lib.load()
    p = lambda k: ctypes.c_void_p(at.get(k, ptr))
    if recs is None:
        recs = A.pack_params(A.identity_params(B, H, W), H, W) if B > 0 and H > 0 and W > 0 else torch.zeros(16, dtype=torch.int32)
    strides = strides or (3 * H * W, H * W, W, 1)
    f3 = lambda v: None if v is None else (ctypes.c_float * 3)(*v)
    rc = lib.dg_augment_forward(p("img"), *strides, ctypes.c_void_p(recs.data_ptr()) if at.get("recs_ptr", 1) else None, p("params"), f3(mean),
                                f3(std), B, C, H, W, h, w, p("img_aug"), p("coord_aug"), p("ws"), ws_bytes, None)
    return rc, lib.dg_last_error().decode()


def test_c_abi_refusals_name_their_reason():
    for kw in (dict(B=0), dict(H=0), dict(w=-1)):
        rc, msg = _forward(**kw)
        assert rc == -1 and "positive" in msg, (kw, rc, msg)
    for kw, word in ((dict(C=4), "channels"), (dict(C=1), "channels"), (dict(H=2), "three pixels"), (dict(W=2), "three pixels"),
                     (dict(h=2), "three pixels"), (dict(B=65536), "65535"), (dict(w=16388), "16384"),
                     (dict(strides=(3 * 256, 256, 1, 16)), "contiguous"), (dict(strides=(3 * 256 + 4, 256, 16, 1)), "contiguous")):
        rc, msg = _forward(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    for box in ((0, 0, 17, 16), (1, 0, 16, 16), (0, 5, 16, 12), (-1, 0, 8, 8), (0, 0, 0, 8)):
        recs = A.pack_params(_params(2, 16, 16, box=[[0, 0, 16, 16], list(box)]), 16, 16)
        rc, msg = _forward(recs=recs)
        assert rc == -2 and "leaves the 16x16 image" in msg and "image 1" in msg, (box, rc, msg)
    rc, msg = _forward(recs=A.pack_params(_params(2, 16, 16, ops=[[1, 0, 1, -1], [-1] * 4]), 16, 16))
    assert rc == -2 and "contrast" in msg
    rc, msg = _forward(recs=A.pack_params(_params(2, 16, 16, ops=[[4, 0, 1, -1], [-1] * 4]), 16, 16))
    assert rc == -1 and "op 4" in msg
    rc, msg = _forward(recs=A.pack_params(_params(2, 16, 16, blur_sigma=[0.5, -1.0]), 16, 16))
    assert rc == -1 and "sigma" in msg
    rc, msg = _forward(ptr=0)
    assert rc == -1 and "null" in msg
    rc, msg = _forward(recs_ptr=0)
    assert rc == -1 and "null" in msg
    for kw in (dict(ws=24), dict(img=18), dict(img_aug=6), dict(coord_aug=10), dict(params=2)):
        rc, msg = _forward(**kw)
        assert rc == -1 and "aligned" in msg, (kw, msg)
    rc, msg = _forward(ws_bytes=255)
    assert rc == -3 and "workspace" in msg
    rc, msg = _forward(mean=(0.5, 0.5, 0.5))
    assert rc == -1 and "together" in msg
    rc, msg = _forward(mean=(0.5, 0.5, 0.5), std=(0.2, 0.0, 0.2))
    assert rc == -1 and "std" in msg


def test_python_refusals_name_their_reason():
    img = torch.rand(2, 3, 8, 8)
    with pytest.raises(ValueError, match="leaves the 8x8 image"):
        A.augment_batch(img, _params(2, 8, 8, box=[[0, 0, 8, 8], [0, 1, 8, 8]]))
    with pytest.raises(ValueError, match="3 channels"):
        A.augment_batch(torch.rand(2, 4, 8, 8), A.identity_params(2, 8, 8))
    with pytest.raises(ValueError, match="three pixels"):
        A.augment_batch(torch.rand(2, 3, 2, 8), A.identity_params(2, 2, 8))
    with pytest.raises(ValueError, match="three pixels"):
        A.augment_batch(img, A.identity_params(2, 8, 8), out_size=(8, 2))
    with pytest.raises(ValueError, match=r"\(3,\) for a batch of 3"):
        A.augment_batch(torch.rand(3, 3, 8, 8), A.identity_params(2, 8, 8))
    with pytest.raises(ValueError, match="two contrast ops"):
        A.augment_batch(img, _params(2, 8, 8, ops=[[1, 1, -1, -1], [-1] * 4]))
    with pytest.raises(ValueError, match="op ids"):
        A.augment_batch(img, _params(2, 8, 8, ops=[[5, 1, -1, -1], [-1] * 4]))
    with pytest.raises(ValueError, match="blur_sigma"):
        A.augment_batch(img, _params(2, 8, 8, blur_sigma=[-0.5, 0.0]))
    with pytest.raises(ValueError, match="together"):
        A.augment_batch(img, A.identity_params(2, 8, 8), mean=A.IMAGENET_MEAN)
    with pytest.raises(ValueError, match="float32"):
        A.augment_batch(img.double(), A.identity_params(2, 8, 8))
    with pytest.raises(TypeError, match="AugmentParams"):
        A.augment_batch(img, (1, 2, 3))
    with pytest.raises(ValueError, match="CPU generator"):
        A.draw_augment_params(2, 8, 8, generator=type("G", (), {"device": torch.device("cuda")})())
    from depthg_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.augment_forward(img, A.pack_params(A.identity_params(2, 8, 8), 8, 8), (8, 8))
