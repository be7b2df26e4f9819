"""GPU tests of the batch augmentation (augment.augment_batch on GPU tensors: dg_augment_forward, dg_augment.hip) against the float64
restatement (tests/augment_reference.py), with the float32 torch chain on the GPU (augment.augment_batch_torch, the CPU route's code
run image by image on GPU tensors) as the yardstick.

MARGIN: per image, both error figures of the kernels - max-abs and relative L2 against the restatement - may be at most MARGIN x the
yardstick's, 2: what the augmentation-alignment and reconstruction terms' tests hold.  The kernels' float32 op order differs from
torch's in the blur (summed in fp64 there) and in hue's division by 6 (torch multiplies by a rounded 1 / 6 on the GPU); the image mean is
fp64 here, which can only help.
Where the yardstick's error is exactly 0 (the identity record, a pure flip, a full-box crop) the kernels must give its bits.
coord_aug is held bit for bit against aug_loss.crop_flip_coords (against the CPU route where the output size differs from the image's,
which crop_flip_coords does not make; tests/test_augment_cpu.py holds that route to crop_flip_coords)."""
import itertools

import pytest
import torch

import augment_reference as R
from depthg_amd import augment as A
from depthg_amd.aug_loss import crop_flip_coords

MARGIN = 2.0
# (B, H, W) -> (h, w), and per image (flip, box): top-left, bottom-right, full and one-pixel-short crops; 8 x 8 lies in one tile, so the
# reflect pad touches both sides; 33 x 47 and 24 x 56 cross tile edges in both directions with a ragged last tile
SHAPES = {
    "5x5": ((1, 5, 5), (5, 5), [(True, (0, 0, 4, 4))]),
    "8x8": ((2, 8, 8), (8, 8), [(False, (0, 0, 8, 8)), (True, (1, 1, 7, 7))]),
    "33x47": ((3, 33, 47), (33, 47), [(True, (0, 0, 27, 40)), (False, (5, 9, 28, 38)), (True, (0, 1, 33, 46))]),
    "40x40": ((2, 40, 40), (24, 56), [(False, (0, 0, 24, 40)), (True, (16, 2, 24, 38))]),
}
KINDS = ("brightness", "contrast", "saturation", "hue", "gray", "blur")


def inputs(shape, seed=0):
    """img in [0.02, 0.98]: a hue-first order stays where the reference's formula is finite."""
    (B, H, W), _, _ = SHAPES[shape]
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(100 + seed)) * 0.96 + 0.02


def params(shape, kind):
    (B, H, W), _, geo = SHAPES[shape]
    p = A.identity_params(B, H, W)
    p.flip[:] = torch.tensor([f for f, _ in geo])
    p.box[:] = torch.tensor([b for _, b in geo], dtype=torch.int32)
    p.factors[:] = torch.tensor([[1.27, 0.74, 1.21, -0.083], [0.71, 1.3, 0.7, 0.1], [1.1, 0.9, 1.3, 0.047]])[:B]
    if kind in KINDS[:4]:
        p.ops[:, 0] = KINDS.index(kind)
    elif kind == "gray":
        p.gray[:] = True
    elif kind == "blur":
        p.blur_sigma[:] = torch.tensor([0.35, 2.0, 0.9])[:B]
    return p


def orders_case():
    """B = 24 at 16 x 16: every order of the four ops, gray and blur mixed in, flips and crops mixed."""
    g = torch.Generator().manual_seed(7)
    p = A.draw_augment_params(24, 16, 16, g, p_gray=0.3, p_blur=0.6)
    p.ops[:] = torch.tensor(list(itertools.permutations(range(4))), dtype=torch.int8)
    return torch.rand(24, 3, 16, 16, generator=g) * 0.96 + 0.02, p


def test_inputs_stay_where_the_hue_formula_is_finite():
    for shape in SHAPES:
        x = inputs(shape)
        assert float(x.min()) >= 0.02 and float(x.max()) <= 0.98
    x, p = orders_case()
    assert float(x.min()) >= 0.02 and float(x.max()) <= 0.98
    assert {tuple(o) for o in p.ops.tolist()} == set(itertools.permutations(range(4)))
    assert bool(p.gray.any()) and not bool(p.gray.all()) and bool((p.blur_sigma > 0).any()) and not bool((p.blur_sigma > 0).all())
    for shape, ((B, H, W), _, geo) in SHAPES.items():
        assert len(geo) == B


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def check(img, p, dev, out_size=None, label="", **space):
    """The criterion of the module docstring on one case; returns the kernels' (img_aug, coord_aug)."""
    truth = R.augment(img, p, out_size, **space)
    got, coord = A.augment_batch(img.to(dev), p, out_size=out_size, **space)
    yard, yard_coord = A.augment_batch_torch(img.to(dev), p, out_size=out_size, **space)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(truth.shape) and bool(torch.isfinite(got).all())
    k_max, k_rel = R.errors(got, truth)
    y_max, y_rel = R.errors(yard, truth)
    for b in range(img.shape[0]):
        print(f"{label} image {b}: max-abs kernel {float(k_max[b]):.3e} yardstick {float(y_max[b]):.3e} | rel-L2 kernel {float(k_rel[b]):.3e} "
              f"yardstick {float(y_rel[b]):.3e}")
    for b in range(img.shape[0]):
        if float(y_max[b]) == 0.0:
            assert torch.equal(got[b], yard[b]), f"{label} image {b}: the yardstick is exact, the kernels are not"
        else:
            assert float(k_max[b]) <= MARGIN * float(y_max[b]), (label, b, float(k_max[b]), float(y_max[b]))
            assert float(k_rel[b]) <= MARGIN * float(y_rel[b]), (label, b, float(k_rel[b]), float(y_rel[b]))
    B, _, H, W = img.shape
    if out_size is None or tuple(out_size) == (H, W):
        want = crop_flip_coords(B, H, W, [tuple(b) for b in p.box.tolist()], p.flip.tolist())
    else:
        want = A.augment_batch(img, p, out_size=out_size, **space)[1]
    assert coord.dtype == torch.float32 and torch.equal(coord.cpu(), want), f"{label}: coord_aug"
    assert torch.equal(yard_coord.cpu(), want)
    return got, coord


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_each_op_alone_within_the_yardsticks_margin(shape, kind, dev):
    check(inputs(shape), params(shape, kind), dev, SHAPES[shape][1], f"{shape}/{kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_geometry_alone_gives_the_yardsticks_bits_where_it_is_exact(shape, dev):
    """No op: flip, crop and resize only.  The identity record returns img and the dataset grid bit for bit."""
    check(inputs(shape), params(shape, "none"), dev, SHAPES[shape][1], f"{shape}/geometry")
    (B, H, W), _, _ = SHAPES[shape]
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1))
    got, coord = A.augment_batch(img.to(dev), A.identity_params(B, H, W))
    assert torch.equal(got.cpu(), img) and torch.equal(coord.cpu(), R.dataset_grid(B, H, W))
    flipped = A.identity_params(B, H, W)
    flipped.flip[:] = True
    got, coord = A.augment_batch(img.to(dev), flipped)
    assert torch.equal(got.cpu(), img.flip(-1)) and torch.equal(coord.cpu(), R.dataset_grid(B, H, W).flip(2))


@pytest.mark.gpu
def test_all_24_orders_with_gray_and_blur_mixed(dev):
    img, p = orders_case()
    check(img, p, dev, None, "orders")


@pytest.mark.gpu
def test_normalised_input_with_mean_and_std(dev):
    img, p = orders_case()
    mean, std = (torch.tensor(v).view(1, 3, 1, 1) for v in (A.IMAGENET_MEAN, A.IMAGENET_STD))
    check(((img - mean) / std)[:8], A.AugmentParams(*(t[8:16] for t in p)), dev, None, "unit", mean=A.IMAGENET_MEAN, std=A.IMAGENET_STD)


@pytest.mark.gpu
def test_out_of_range_input_is_clamped_by_a_leading_brightness(dev):
    img, p = orders_case()
    img = torch.randn(24, 3, 16, 16, generator=torch.Generator().manual_seed(8)) * 1.5 + 0.3
    first = [o for o in itertools.permutations(range(4)) if o[0] == A.BRIGHTNESS]
    q = A.AugmentParams(*(t[:6].clone() for t in p))
    q.ops[:] = torch.tensor(first, dtype=torch.int8)
    assert float(img.min()) < -1.0 and float(img.max()) > 2.0
    got, _ = check(img[:6], q, dev, None, "clamp")
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 + 1e-6


@pytest.mark.gpu
def test_two_calls_give_the_same_bits_and_poison_changes_nothing(dev, monkeypatch):
    from depthg_amd import ops
    img, p = orders_case()
    x = img.to(dev)
    a = A.augment_batch(x, p)
    b = A.augment_batch(x, p)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    monkeypatch.setattr(ops, "POISON", True)             # workspace and outputs start as 0xFF bytes
    c = A.augment_batch(x, p, out_size=(17, 22))
    monkeypatch.setattr(ops, "POISON", False)
    d = A.augment_batch(x, p, out_size=(17, 22))
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and bool(torch.isfinite(c[0]).all()) and bool(torch.isfinite(c[1]).all())
    # a view of a larger buffer is copied once and gives the bits of its contiguous copy; params on the GPU are taken too
    big = torch.zeros(24, 3, 16, 20, device=dev)
    big[..., 2:18] = x
    e = A.augment_batch(big[..., 2:18], A.AugmentParams(*(t.to(dev) for t in p)))
    assert torch.equal(e[0], a[0]) and torch.equal(e[1], a[1])


@pytest.mark.gpu
def test_the_statistics_launch_is_per_image_clean(dev):
    """A batch with no contrast op anywhere, and the same batch with a contrast op of factor 1 appended to one image: the statistics
    kernel runs in the second call only, and no other image may see it (nor, at factor 1 on [0, 1] values, the image itself)."""
    img = inputs("33x47").to(dev)
    p = params("33x47", "saturation")
    p.blur_sigma[:] = torch.tensor([0.0, 1.1, 0.6])
    assert not bool((p.ops == A.CONTRAST).any())
    q = A.AugmentParams(*(t.clone() for t in p))
    q.ops[1, 1] = A.CONTRAST
    q.factors[1, A.CONTRAST] = 1.0
    a, b = A.augment_batch(img, p), A.augment_batch(img, q)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_gpu_refusals(dev):
    x = torch.rand(2, 3, 8, 8, device=dev)
    with pytest.raises(ValueError, match="float32"):
        A.augment_batch(x.double(), A.identity_params(2, 8, 8))
    with pytest.raises(ValueError, match="three pixels"):
        A.augment_batch(x, A.identity_params(2, 8, 8), out_size=(2, 8))
    with pytest.raises(ValueError, match="leaves the 8x8 image"):
        bad = A.identity_params(2, 8, 8)
        bad.box[1, 3] = 9
        A.augment_batch(x, bad)


def _step(dev, gpu_augment, make_extra=None):
    """One seeded training_step under cfg.aug_alignment_weight = 0.5; make_extra(batch): further batch entries, made behind the seeding
    from the global generator - where the keyed step makes its draw."""
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(4)
    cfg = default_segmenter_cfg(res=32, correspondence_weight=0.0, aug_alignment_weight=0.5)
    if gpu_augment:
        cfg.dg_gpu_augment = gpu_augment
    m = UnsupervisedSegmenter(5, cfg).to(dev)
    m.train()
    g = torch.Generator().manual_seed(0)
    batch = {"img": torch.rand(2, 3, 32, 32, generator=g).to(dev), "img_pos": torch.rand(2, 3, 32, 32, generator=g).to(dev),
             "label": torch.randint(0, 5, (2, 32, 32), generator=g).to(dev), "depth": torch.rand(2, 1, 32, 32, generator=g).to(dev),
             "depth_pos": torch.rand(2, 1, 32, 32, generator=g).to(dev)}
    torch.manual_seed(6)
    torch.cuda.manual_seed(6)
    if make_extra is not None:
        batch.update(make_extra(batch))
    loss, logs = m.training_step(batch, 0)
    torch.cuda.synchronize()
    return loss, logs, [p.grad.detach().clone() for p in m.head_parameters()]


@pytest.mark.gpu
def test_training_step_with_the_key_equals_a_step_fed_augment_batchs_tensors(dev):
    def fed(batch, **space):
        img_aug, coord_aug = A.augment_batch(batch["img"], A.draw_augment_params(2, 32, 32), **space)
        return {"img_aug": img_aug, "coord_aug": coord_aug}

    for key, space in ((True, {}), ("unit", dict(mean=A.IMAGENET_MEAN, std=A.IMAGENET_STD))):
        loss_a, logs_a, grads_a = _step(dev, key)
        loss_b, logs_b, grads_b = _step(dev, False, lambda batch: fed(batch, **space))
        assert "loss/aug_alignment" in logs_a and bool(torch.isfinite(loss_a))
        assert torch.equal(logs_a["loss/aug_alignment"], logs_b["loss/aug_alignment"]) and torch.equal(loss_a, loss_b)
        assert len(grads_a) > 0 and all(torch.equal(x, y) for x, y in zip(grads_a, grads_b))
    with pytest.raises(KeyError, match="img_aug"):
        _step(dev, False)
