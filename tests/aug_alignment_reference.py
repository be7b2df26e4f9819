"""The augmentation-alignment term (src/train_segmentation.py:400-411) restated in float64 from its formulas, with analytic gradients -
the truth the CPU and GPU tests measure against - and the input makers both share.

    ds   = resize(coord_aug.permute(0,3,1,2), n).permute(0,2,3,1)          bilinear, align_corners=False
    u    = sample(code, ds):  u[b,:,i,j] reads x = ds[b,j,i,0], y = ds[b,j,i,1]  bilinear, border, align_corners=True
    s    = <u / max(|u|, eps), v / max(|v|, eps)>,  v = code_aug[b,:,i,j],     loss = -mean s
    d v  = c (u^ - s v^) / |v|,  d u = c (v^ - s u^) / |u|,  c = -1 / (B n^2)    where the norm is >= eps;
    d v  = c u^ / eps,           d u = c v^ / eps                               below it (F.normalize's clamp_min(|x|, eps) is a
                                                                                constant there under autograd; x^ = x / eps)
    d code = the adjoint of the bilinear taps applied to d u.
Nothing here calls F.interpolate, F.grid_sample, F.normalize or autograd: torch_chain() below is that chain (the yardstick's).
"""
import functools
import math

import torch
import torch.nn.functional as F

EPS = 1e-10
B = 2
# name: (D, (h, w) of code, n of code_aug, (H, W) of coord_aug)
SHAPES = {
    "tiny": (5, (4, 4), 3, (24, 24)),               # less than one wave of positions
    "nonsquare": (5, (7, 9), 6, (40, 72)),          # non-square source and image
    "upsample": (33, (6, 6), 20, (20, 20)),         # many positions per pixel, a coordinate resize that is the identity
    "reference": (70, (28, 28), 28, (224, 224)),    # the reference's shape
    "wide": (128, (14, 14), 14, (112, 112)),        # wide D
    "large": (70, (56, 56), 56, (448, 448)),        # the largest tap records
}
KINDS = ("cropflip", "identity", "scaled", "equal", "centres")
CASES = [(shape, "cropflip") for shape in SHAPES] + [(shape, kind) for shape in ("nonsquare", "reference") for kind in KINDS[1:]]
# One more for the GPU alone: 5 x ceil(58^2 / 64) = 265 blocks of k_aug_forward, more partial sums than k_loss_reduce has threads
# (8 * 64 + 24 * 3364 + 4 bytes of LDS for the tap records).  Not in CASES: with D = 3 some of its 16820 positions have s next to
# +-1, which test_gpu_cases_have_gradients_far_above_rounding rules out position by position; the whole gradients, which the GPU
# test measures, are as far above rounding as the others'.  (The name sorts last: inputs() seeds by the sorted position.)
SHAPES["wraps"] = (3, (8, 8), 58, (64, 64))
BATCH = {"wraps": 5}                                # images, where not B
WRAPS_CASE = ("wraps", "cropflip")


def _resize_axis(size_in, size_out):
    dst = torch.arange(size_out, dtype=torch.float64)
    src = ((dst + 0.5) * (size_in / size_out) - 0.5).clamp(min=0.0)
    i0 = src.floor().long().clamp(max=size_in - 1)
    return i0, (i0 + 1).clamp(max=size_in - 1), src - i0


def downsample_coords(coord_aug, n):
    """(B,H,W,2) -> ds (B,n,n,2) in float64."""
    c = coord_aug.double()
    r0, r1, lr = _resize_axis(c.shape[1], n)
    c0, c1, lc = _resize_axis(c.shape[2], n)
    rows = c[:, r0] * (1 - lr)[None, :, None, None] + c[:, r1] * lr[None, :, None, None]
    return rows[:, :, c0] * (1 - lc)[None, None, :, None] + rows[:, :, c1] * lc[None, None, :, None]


def taps(ds, h, w):
    """The four (pixel, weight) taps of every output position p = i * n + j: idx (B,P,4) int64 into the flattened map, wts (B,P,4)."""
    g = ds.transpose(1, 2)                                        # g[b,i,j,:] = ds[b,j,i,:]
    x = ((g[..., 0] + 1) / 2 * (w - 1)).clamp(0, w - 1).flatten(1)
    y = ((g[..., 1] + 1) / 2 * (h - 1)).clamp(0, h - 1).flatten(1)
    x0, y0 = x.floor(), y.floor()
    fx, fy = x - x0, y - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    idx = torch.stack([y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1], -1)
    wts = torch.stack([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx], -1)
    return idx, wts


def chain(code, code_aug, coord_aug):
    """dict(loss, d_code, d_code_aug, s (B,n,n), u (B,D,n,n), mean_abs_s), float64, for an upstream gradient of 1."""
    code, code_aug = code.double(), code_aug.double()
    Bn, D, h, w = code.shape
    n = code_aug.shape[2]
    P = n * n
    idx, wts = taps(downsample_coords(coord_aug, n), h, w)
    flat = idx.reshape(Bn, 1, 4 * P).expand(Bn, D, 4 * P)
    u = (code.flatten(2).gather(2, flat).view(Bn, D, P, 4) * wts[:, None]).sum(-1)             # (B,D,P)
    v = code_aug.flatten(2)
    nu, nv = u.square().sum(1).sqrt(), v.square().sum(1).sqrt()                                 # (B,P)
    uh, vh = u / nu.clamp(min=EPS)[:, None], v / nv.clamp(min=EPS)[:, None]
    s = (uh * vh).sum(1)
    c = -1.0 / (Bn * P)
    d_v = torch.where((nv >= EPS)[:, None], c * (uh - s[:, None] * vh) / nv.clamp(min=EPS)[:, None], c * uh / EPS)
    d_u = torch.where((nu >= EPS)[:, None], c * (vh - s[:, None] * uh) / nu.clamp(min=EPS)[:, None], c * vh / EPS)
    d_code = torch.zeros(Bn, D, h * w, dtype=torch.float64)
    d_code.scatter_add_(2, flat, (d_u[..., None] * wts[:, None]).reshape(Bn, D, 4 * P))
    return {"loss": float(-s.mean()), "d_code": d_code.view(Bn, D, h, w), "d_code_aug": d_v.view(Bn, D, n, n), "s": s.view(Bn, n, n),
            "u": u.view(Bn, D, n, n), "mean_abs_s": float(s.abs().mean())}


def torch_chain(code, code_aug, coord_aug):
    """The reference's chain in torch, differentiable, in the tensors' dtype and on their device."""
    n = code_aug.shape[2]
    ds = F.interpolate(coord_aug.permute(0, 3, 1, 2), (n, n), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    u = F.grid_sample(code, ds.permute(0, 2, 1, 3), padding_mode="border", align_corners=True)
    return -torch.einsum("bkhw,bkhw->bhw", F.normalize(u, dim=1, eps=1e-10), F.normalize(code_aug, dim=1, eps=1e-10)).mean()


def spacing32(x):
    """One float32 spacing at the magnitude of x."""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x != 0 else 2.0 ** -149


def dataset_grid(Bn, H, W):
    """src/data.py:1085-1087, 1139: (B,H,W,2), channel 0 the row coordinate."""
    rows, cols = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    return torch.stack([rows, cols], -1)[None].expand(Bn, H, W, 2).contiguous()


def make_coords(kind, h, w, n, H, W, gen, B=B):
    from depthg_amd.aug_loss import crop_flip_coords
    full = [(0, 0, H, W)] * B
    if kind == "cropflip":                 # boxes of 0.8 .. 1.0 of the area, every other image flipped
        boxes = []
        for _ in range(B):
            side = math.sqrt(0.8 + 0.2 * float(torch.rand((), generator=gen)))
            bh, bw = H * side, W * side
            boxes.append((float(torch.rand((), generator=gen)) * (H - bh), float(torch.rand((), generator=gen)) * (W - bw), bh, bw))
        return crop_flip_coords(B, H, W, boxes, [b % 2 == 1 for b in range(B)])
    if kind == "identity":
        return crop_flip_coords(B, H, W, full, [False] * B)
    if kind == "scaled":                   # coordinates leave [-1, 1]: the border clamp and the edge taps act
        return crop_flip_coords(B, H, W, full, [False] * B) * 1.3
    if kind == "equal":                    # one pixel neighbourhood's inverse lists hold every position
        return torch.tensor([0.31, -0.45]).expand(B, H, W, 2).contiguous()
    if kind == "centres":
        # every resized coordinate on a pixel centre of the code map - the corners and the middle exactly, the others to within
        # one float32 spacing - so taps of weight zero occur: centres on the (n, n) grid, spread to (H, W) by nearest-neighbour
        # repetition (the bilinear resize back to (n, n) then blends equal values)
        kx, ky = torch.randint(0, w, (B, n, n), generator=gen), torch.randint(0, h, (B, n, n), generator=gen)
        kx[:, 0, 0], ky[:, 0, 0], kx[:, 0, 1], ky[:, 0, 1] = 0, 0, w - 1, h - 1
        kx[:, 1, 0], ky[:, 1, 0], kx[:, 1, 1], ky[:, 1, 1] = w - 1, 0, 0, h - 1
        grid = torch.stack([2.0 * kx / (w - 1) - 1.0, 2.0 * ky / (h - 1) - 1.0], 1).float()            # (B,2,n,n): channel 0 is read as x
        return F.interpolate(grid, (H, W), mode="nearest").permute(0, 2, 3, 1).contiguous()
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    """(code, code_aug, coord_aug) on the CPU, float32: independent random maps with a mean offset, so that s stays away from +-1 and
    both true gradients are far above rounding."""
    D, (h, w), n, (H, W) = SHAPES[shape]
    gen = torch.Generator().manual_seed(1000 + 10 * sorted(SHAPES).index(shape) + KINDS.index(kind))
    Bn = BATCH.get(shape, B)
    code = torch.randn(Bn, D, h, w, generator=gen) + 0.6
    code_aug = torch.randn(Bn, D, n, n, generator=gen) + 0.6
    return code, code_aug, make_coords(kind, h, w, n, H, W, gen, Bn)


@functools.lru_cache(maxsize=None)
def truth(shape, kind):
    """chain() of inputs(shape, kind), once per case - shared by the tests, never modified."""
    return chain(*inputs(shape, kind))
