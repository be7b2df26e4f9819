"""GPU batch augmentation: the augmented view and the coordinate map the augmentation-alignment term reads (cfg.aug_alignment_weight),
which the reference makes per sample on CPU workers (ContrastiveSegDataset.__getitem__, src/data.py:1082-1139, with the transforms of
src/train_segmentation.py:602-610): RandomHorizontalFlip, RandomResizedCrop(res, scale=(0.8, 1.0)), ColorJitter(.3, .3, .3, .1),
RandomGrayscale(.2), RandomApply([GaussianBlur((5, 5))]) on the image, and the geometric pair again on the coordinate grid.

    draw_augment_params(B, H, W, generator=None, ...)   an AugmentParams record of CPU tensors, B rows each
    augment_batch(img, params, out_size=None, mean=None, std=None)   (img_aug (B,3,h,w), coord_aug (B,h,w,2)), both float32

Per image, the arithmetic of torchvision's tensor transforms:
  geometry   the flip, then the crop `box`, then a plain bilinear resize to (h, w) (align_corners=False, taps held inside the crop).  A
             box never exceeds the image, so this is never a down-scale and antialiasing does not arise.  coord_aug is the dataset's
             grid (channel 0 = linspace(-1, 1, H) down the rows, channel 1 = linspace(-1, 1, W) along the columns) under the same
             flip, crop and resize: aug_loss.crop_flip_coords's rule and bits.  Source positions are fp64, the blends float32.
  colour     mean=None (the reference's behaviour): the ops act on the tensor as given - the reference feeds them the
             ImageNet-normalised image, and their clamps to [0, 1] act on those values.  With mean / std (three values each) the pixel
             is de-normalised behind the resize (x * std + mean) and re-normalised at the very end ((x - mean) / std).
  ops        in the record's slot order: brightness clamp(f x, 0, 1); contrast clamp(f x + (1 - f) m, 0, 1), m the mean over the image
             of gray(x) as the image stands when the op's turn comes; saturation clamp(f x + (1 - f) gray(x), 0, 1); hue:
             torchvision's _rgb2hsv, h = (h + f) mod 1, _hsv2rgb (its p, q and t clamped to [0, 1], v as it is); gray(x) = 0.2989 r +
             0.587 g + 0.114 b.  Then RandomGrayscale (the three channels become the gray), then the 5 x 5 blur: the outer product
             of exp(-0.5 (x / sigma)^2) on x = -2..2, normalised, over the reflect-padded image.
On CPU tensors augment_batch is that chain in plain float32 torch, one image at a time.  On GPU tensors it is two HIP launches for the
whole batch (ops.augment_forward, dg_augment.hip), whatever B is; `params` may live on either device and is uploaded once, as one small
tensor.  The same chain on GPU tensors, image by image, is `augment_batch_torch`: the yardstick of the tests and of the timing script.
"""
import math
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from . import ops

BRIGHTNESS, CONTRAST, SATURATION, HUE, NO_OP = 0, 1, 2, 3, -1
IMAGENET_MEAN, IMAGENET_STD = ops.IMAGENET_MEAN, ops.IMAGENET_STD      # the normalisation depthg_amd/demo.py applies


class AugmentParams(NamedTuple):
    """B rows each.  flip: bool (B,).  box: int32 (B, 4) = (top, left, height, width) in whole pixels of the flipped image.  ops: int8
    (B, 4), the op of each slot (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none), applied in slot order.  factors: float32
    (B, 4) indexed by op id.  gray: bool (B,).  blur_sigma: float32 (B,), 0 = no blur."""
    flip: torch.Tensor
    box: torch.Tensor
    ops: torch.Tensor
    factors: torch.Tensor
    gray: torch.Tensor
    blur_sigma: torch.Tensor


def identity_params(B, H, W):
    """The record that changes nothing: no flip, the full box, four empty slots, no gray, no blur."""
    return AugmentParams(torch.zeros(B, dtype=torch.bool), torch.tensor([[0, 0, H, W]] * B, dtype=torch.int32).reshape(B, 4),
                         torch.full((B, 4), NO_OP, dtype=torch.int8), torch.tensor([[1.0, 1.0, 1.0, 0.0]] * B).reshape(B, 4),
                         torch.zeros(B, dtype=torch.bool), torch.zeros(B))


def draw_augment_params(B, H, W, generator=None, *, scale=(0.8, 1.0), ratio=(3 / 4, 4 / 3), brightness=.3, contrast=.3, saturation=.3,
                        hue=.1, p_flip=.5, p_gray=.2, p_blur=.5, sigma=(0.1, 2.0)):
    """The parameters of B augmentations of (H, W) images, drawn from the CPU generator `generator` (default: torch's global one); the
    defaults are the reference's values.  Per image the draws follow torchvision's order of calls:
      1. rand(1) < p_flip                                                        (RandomHorizontalFlip)
      2. the crop (RandomResizedCrop.get_params): up to ten tries of  area x uniform(scale),  exp(uniform(log ratio)),  the rounded
         w and h, accepted when 0 < w <= W and 0 < h <= H, then randint for top and for left;  if none is accepted, the centre crop
         at the clamped ratio
      3. randperm(4), then uniform for brightness, contrast, saturation, hue     (ColorJitter.get_params)
      4. rand(1) < p_gray                                                        (RandomGrayscale)
      5. rand(1) for the blur, then uniform(sigma)                               (RandomApply([GaussianBlur]); sigma only if applied)
    Reproducing torchvision's random stream bit for bit is NOT claimed: torchvision is not a dependency and the claim cannot be
    checked without it.  What is promised is the order above, the distributions, and that equal generator states give equal records."""
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"depthg_amd: draw_augment_params wants B, H, W >= 1, got {B}, {H}, {W}")
    if generator is not None and generator.device.type != "cpu":
        raise ValueError("depthg_amd: draw_augment_params draws from a CPU generator")
    g = generator

    def rand():
        return float(torch.rand(1, generator=g))

    def uniform(lo, hi):
        return float(torch.empty(1).uniform_(lo, hi, generator=g))

    def randint(hi):                       # [0, hi]
        return int(torch.randint(0, hi + 1, (1,), generator=g))

    flip, box, slots, factors, gray, sig = [], [], [], [], [], []
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(B):
        flip.append(rand() < p_flip)
        area = H * W
        for _try in range(10):
            target = area * uniform(scale[0], scale[1])
            aspect = math.exp(uniform(log_ratio[0], log_ratio[1]))
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= W and 0 < h <= H:
                top = randint(H - h)
                left = randint(W - w)
                break
        else:
            in_ratio = W / H
            if in_ratio < min(ratio):
                w, h = W, int(round(W / min(ratio)))
            elif in_ratio > max(ratio):
                h, w = H, int(round(H * max(ratio)))
            else:
                w, h = W, H
            h, w = max(1, min(h, H)), max(1, min(w, W))
            top, left = (H - h) // 2, (W - w) // 2
        box.append((top, left, h, w))
        slots.append(torch.randperm(4, generator=g).tolist())
        factors.append((uniform(max(0.0, 1 - brightness), 1 + brightness), uniform(max(0.0, 1 - contrast), 1 + contrast),
                        uniform(max(0.0, 1 - saturation), 1 + saturation), uniform(-hue, hue)))
        gray.append(rand() < p_gray)
        sig.append(uniform(sigma[0], sigma[1]) if rand() < p_blur else 0.0)
    return AugmentParams(torch.tensor(flip, dtype=torch.bool), torch.tensor(box, dtype=torch.int32).reshape(B, 4),
                         torch.tensor(slots, dtype=torch.int8).reshape(B, 4), torch.tensor(factors, dtype=torch.float32).reshape(B, 4),
                         torch.tensor(gray, dtype=torch.bool), torch.tensor(sig, dtype=torch.float32))


def _checked(params, B, H, W):
    """`params` on the CPU in its dtypes, B rows, every box inside the (H, W) image and every record one the kernels take."""
    if not isinstance(params, AugmentParams):
        raise TypeError(f"depthg_amd: augment_batch wants an AugmentParams record, got {type(params).__name__}")
    p = AugmentParams(params.flip.detach().cpu().to(torch.bool), params.box.detach().cpu().to(torch.int32), params.ops.detach().cpu().to(torch.int8),
                      params.factors.detach().cpu().to(torch.float32), params.gray.detach().cpu().to(torch.bool),
                      params.blur_sigma.detach().cpu().to(torch.float32))
    shapes = ((B,), (B, 4), (B, 4), (B, 4), (B,), (B,))
    for name, t, shape in zip(AugmentParams._fields, p, shapes):
        if tuple(t.shape) != shape:
            raise ValueError(f"depthg_amd: params.{name} must be {shape} for a batch of {B}, got {tuple(t.shape)}")
    top, left, bh, bw = (p.box[:, k].long() for k in range(4))
    bad = ~((bh > 0) & (bw > 0) & (top >= 0) & (left >= 0) & (top + bh <= H) & (left + bw <= W))
    if bool(bad.any()):
        b = int(bad.nonzero()[0])
        raise ValueError(f"depthg_amd: crop box {tuple(p.box[b].tolist())} of image {b} leaves the {H}x{W} image")
    if bool(((p.ops < NO_OP) | (p.ops > HUE)).any()):
        raise ValueError(f"depthg_amd: params.ops holds op ids -1 (none) .. 3, got {sorted(set(p.ops.flatten().tolist()))}")
    if bool(((p.ops == CONTRAST).sum(1) > 1).any()):
        raise ValueError("depthg_amd: an image has two contrast ops (one image mean per image: one at most)")
    if not bool((torch.isfinite(p.blur_sigma) & (p.blur_sigma >= 0)).all()):
        raise ValueError("depthg_amd: params.blur_sigma must be finite and >= 0 (0: no blur)")
    return p


def _colour_space(mean, std):
    if (mean is None) != (std is None):
        raise ValueError("depthg_amd: augment_batch wants mean and std together: give both or neither")
    if mean is None:
        return None, None
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or not all(s > 0 and math.isfinite(s) for s in std) or not all(math.isfinite(m) for m in mean):
        raise ValueError(f"depthg_amd: mean and std hold three finite values each, std > 0, got {mean} and {std}")
    return mean, std


def _axis_taps(n_out, start, length):
    """Output positions 0..n_out-1 over the crop [start, start + length): the two source pixels and the float32 fraction; the
    position in fp64, as aug_loss.crop_flip_coords forms it."""
    src = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (float(length) / n_out) - 0.5).clamp(0.0, max(float(length) - 1.0, 0.0)) + float(start)
    i0 = src.floor().long()
    i1 = (i0 + 1).clamp(max=start + length - 1)
    return i0, i1, (src - i0).to(torch.float32)


def _gray(x):
    return 0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]


def _blend(x, other, f):
    return (f * x + (1.0 - f) * other).clamp(0.0, 1.0)


def _hue(x, f):
    r, g, b = x[0], x[1], x[2]
    maxc, minc = x.max(0).values, x.min(0).values
    eq = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eq, ones, maxc)
    div = torch.where(eq, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    zero = torch.zeros_like(maxc)
    hr = torch.where(maxc == r, bc - gc, zero)
    hg = torch.where((maxc == g) & (maxc != r), 2.0 + rc - bc, zero)
    hb = torch.where((maxc != g) & (maxc != r), 4.0 + gc - rc, zero)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + f) % 1.0
    h6 = h * 6.0
    fl = torch.floor(h6)
    fr = h6 - fl
    v = maxc
    p = (v * (1.0 - s)).clamp(0.0, 1.0)
    q = (v * (1.0 - s * fr)).clamp(0.0, 1.0)
    t = (v * (1.0 - s * (1.0 - fr))).clamp(0.0, 1.0)
    i = (fl.to(torch.int64) % 6)[None]
    pick = lambda table: torch.gather(torch.stack(table), 0, i)[0]
    return torch.stack((pick((v, q, p, p, t, v)), pick((t, v, v, q, p, p)), pick((p, p, t, v, v, q))))


def _blur(x, sigma):
    k = torch.linspace(-2.0, 2.0, 5, dtype=torch.float32, device=x.device)
    pdf = torch.exp(-0.5 * (k / sigma).pow(2))
    k1 = pdf / pdf.sum()
    k2 = (k1[:, None] * k1[None, :]).expand(3, 1, 5, 5)
    return F.conv2d(F.pad(x[None], (2, 2, 2, 2), mode="reflect"), k2, groups=3)[0]


def _augment_one(x, rows, cols, flip, box, slots, factors, gray, sigma, out_size, mean, std):
    """One image (3, H, W) through the chain, float32, on x's device; rows / cols: the two coordinate ramps on that device."""
    h, w = out_size
    top, left, bh, bw = box
    y0, y1, fy = (t.to(x.device) for t in _axis_taps(h, top, bh))
    x0, x1, fx = (t.to(x.device) for t in _axis_taps(w, left, bw))
    if flip:
        x0, x1 = x.shape[2] - 1 - x0, x.shape[2] - 1 - x1
    coord = torch.empty(h, w, 2, dtype=torch.float32, device=x.device)
    coord[:, :, 0] = (rows[y0] * (1.0 - fy) + rows[y1] * fy)[:, None]
    coord[:, :, 1] = (cols[x0] * (1.0 - fx) + cols[x1] * fx)[None, :]
    ra, rb = x[:, y0], x[:, y1]
    upper = ra[:, :, x0] * (1.0 - fx) + ra[:, :, x1] * fx
    lower = rb[:, :, x0] * (1.0 - fx) + rb[:, :, x1] * fx
    x = upper * (1.0 - fy)[:, None] + lower * fy[:, None]
    if mean is not None:
        x = x * std + mean
    for op in slots:
        if op == BRIGHTNESS:
            x = _blend(x, torch.zeros_like(x), factors[BRIGHTNESS])
        elif op == CONTRAST:
            x = _blend(x, _gray(x).mean(), factors[CONTRAST])
        elif op == SATURATION:
            x = _blend(x, _gray(x)[None], factors[SATURATION])
        elif op == HUE:
            x = _hue(x, factors[HUE])
    if gray:
        x = _gray(x)[None].expand(3, -1, -1)
    if sigma > 0:
        x = _blur(x, sigma)
    if mean is not None:
        x = (x - mean) / std
    return x, coord


def augment_batch_torch(img, params, *, out_size=None, mean=None, std=None):
    """The chain of the module docstring in plain float32 torch, one image at a time, on img's device: augment_batch's CPU route, and on
    GPU tensors the per-image loop the fused route is measured against."""
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"depthg_amd: augment_batch wants img as (B, 3, H, W), got {tuple(img.shape)}: the colour ops are RGB (3 channels)")
    if img.dtype != torch.float32:
        raise ValueError(f"depthg_amd: augment_batch wants a float32 img, got {img.dtype}")
    B, _, H, W = img.shape
    h, w = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if min(H, W, h, w) < 3:
        raise ValueError(f"depthg_amd: image {H}x{W}, output {h}x{w}: reflect padding by 2 needs three pixels a side")
    p = _checked(params, B, H, W)
    mean, std = _colour_space(mean, std)
    if mean is not None:
        mean, std = (torch.tensor(v, dtype=torch.float32, device=img.device).view(3, 1, 1) for v in (mean, std))
    rows, cols = torch.linspace(-1, 1, H).to(img.device), torch.linspace(-1, 1, W).to(img.device)
    img_aug = torch.empty(B, 3, h, w, dtype=torch.float32, device=img.device)
    coord_aug = torch.empty(B, h, w, 2, dtype=torch.float32, device=img.device)
    flips, boxes, slots, factors, grays, sigmas = p.flip.tolist(), p.box.tolist(), p.ops.tolist(), p.factors.tolist(), p.gray.tolist(), p.blur_sigma.tolist()
    img = img.detach()
    for b in range(B):
        img_aug[b], coord_aug[b] = _augment_one(img[b], rows, cols, flips[b], boxes[b], slots[b], factors[b], grays[b], sigmas[b], (h, w), mean, std)
    return img_aug, coord_aug


def pack_params(params, H, W):
    """The record as the library reads it (include/depthg_corr.h, dg_augment_forward): one CPU int32 tensor of B x 16 words - flip, the
    box, the four slots, the four factors' float32 bits, gray, sigma's bits, zero - followed by the bits of linspace(-1, 1, H) and
    linspace(-1, 1, W)."""
    B = params.flip.numel()
    buf = torch.zeros(B * 16 + H + W, dtype=torch.int32)
    rec, recf = buf[:B * 16].view(B, 16), buf[:B * 16].view(torch.float32).view(B, 16)
    rec[:, 0] = params.flip.to(torch.int32)
    rec[:, 1:5] = params.box
    rec[:, 5:9] = params.ops.to(torch.int32)
    recf[:, 9:13] = params.factors
    rec[:, 13] = params.gray.to(torch.int32)
    recf[:, 14] = params.blur_sigma
    ramps = buf[B * 16:].view(torch.float32)
    ramps[:H] = torch.linspace(-1, 1, H)
    ramps[H:] = torch.linspace(-1, 1, W)
    return buf


def augment_batch(img, params, *, out_size: Optional[Tuple[int, int]] = None, mean=None, std=None):
    """(img_aug (B,3,h,w), coord_aug (B,h,w,2)) of img (B,3,H,W) float32 under `params` (see the module docstring); (h, w) defaults to
    (H, W).  CPU tensors: the float32 torch chain.  GPU tensors: two HIP launches for the batch; a non-contiguous img is copied once."""
    if not img.is_cuda:
        return augment_batch_torch(img, params, out_size=out_size, mean=mean, std=std)
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"depthg_amd: augment_batch wants img as (B, 3, H, W), got {tuple(img.shape)}: the colour ops are RGB (3 channels)")
    ops._gpu_float32(((img, "img"),), "augment_batch wants a float32 img on the GPU, got {name} as {dtype}")
    B, _, H, W = img.shape
    h, w = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if min(H, W, h, w) < 3:
        raise ValueError(f"depthg_amd: image {H}x{W}, output {h}x{w}: reflect padding by 2 needs three pixels a side")
    p = _checked(params, B, H, W)
    mean, std = _colour_space(mean, std)
    return ops.augment_forward(img, pack_params(p, H, W), (h, w), mean, std)
