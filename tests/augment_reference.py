"""A float64 restatement of the batch augmentation (depthg_amd/augment.py's module docstring), written without looking at its code
paths: the resize is a pair of dense interpolation matrices, the colour ops are numpy on whole images, the blur is 25 shifted adds
over numpy's reflect pad.  It is the truth the float32 routes' errors are taken against, and carries those error figures."""
import numpy as np
import torch

GRAY = (0.2989, 0.587, 0.114)


def axis_matrix(n_out, start, length, dim, flip=False):
    """(n_out, dim) float64: row o holds the two bilinear weights (align_corners=False, taps held inside the crop
    [start, start + length)) with which output o reads the axis; `flip`: the axis is mirrored before the crop."""
    M = np.zeros((n_out, dim))
    for o in range(n_out):
        s = min(max((o + 0.5) * (length / n_out) - 0.5, 0.0), length - 1.0)
        lo = int(np.floor(s))
        hi = min(lo + 1, length - 1)
        for k, wgt in ((lo, 1.0 - (s - lo)), (hi, s - lo)):
            src = start + k
            M[o, dim - 1 - src if flip else src] += wgt
    return M


def resample(x, flip, box, out_size):
    """x (3, H, W) float64 -> (3, h, w): flip, crop, bilinear resize."""
    top, left, bh, bw = box
    Ry = axis_matrix(out_size[0], top, bh, x.shape[1])
    Rx = axis_matrix(out_size[1], left, bw, x.shape[2], flip)
    return np.einsum("ay,cyx,bx->cab", Ry, x, Rx)


def gray(x):
    return GRAY[0] * x[0] + GRAY[1] * x[1] + GRAY[2] * x[2]


def brightness(x, f):
    return np.clip(f * x, 0.0, 1.0)


def contrast(x, f):
    return np.clip(f * x + (1.0 - f) * gray(x).mean(), 0.0, 1.0)


def saturation(x, f):
    return np.clip(f * x + (1.0 - f) * gray(x)[None], 0.0, 1.0)


def rgb2hsv(x):
    r, g, b = x
    maxc, minc = x.max(0), x.min(0)
    eq = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eq, 1.0, maxc)
    d = np.where(eq, 1.0, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    return np.fmod(h / 6.0 + 1.0, 1.0), s, maxc


def hsv2rgb(h, s, v):
    i = np.floor(6.0 * h)
    f = 6.0 * h - i
    i = i.astype(np.int64) % 6
    p = np.clip(v * (1.0 - s), 0.0, 1.0)
    q = np.clip(v * (1.0 - s * f), 0.0, 1.0)
    t = np.clip(v * (1.0 - s * (1.0 - f)), 0.0, 1.0)
    table = np.array([[v, q, p, p, t, v], [t, v, v, q, p, p], [p, p, t, v, v, q]])          # (channel, sextant, H, W)
    return np.take_along_axis(table, i[None, None], 1)[:, 0]


def hue(x, f):
    h, s, v = rgb2hsv(x)
    return hsv2rgb(np.mod(h + f, 1.0), s, v)


def blur_kernel(sigma):
    k = np.exp(-0.5 * (np.arange(-2, 3) / float(sigma)) ** 2)
    return k / k.sum()


def blur(x, sigma):
    k = blur_kernel(sigma)
    H, W = x.shape[1:]
    padded = np.pad(x, ((0, 0), (2, 2), (2, 2)), mode="reflect")
    out = np.zeros_like(x)
    for dy in range(5):
        for dx in range(5):
            out += k[dy] * k[dx] * padded[:, dy:dy + H, dx:dx + W]
    return out


OPS = (brightness, contrast, saturation, hue)


def augment(img, params, out_size=None, mean=None, std=None):
    """img (B,3,H,W) tensor, params the AugmentParams record -> img_aug (B,3,h,w) float64 tensor."""
    x = img.detach().cpu().double().numpy()
    B, _, H, W = x.shape
    out_size = (H, W) if out_size is None else tuple(out_size)
    res = np.zeros((B, 3) + out_size)
    m = None if mean is None else np.asarray(mean, dtype=np.float32).astype(np.float64).reshape(3, 1, 1)
    s = None if std is None else np.asarray(std, dtype=np.float32).astype(np.float64).reshape(3, 1, 1)
    for b in range(B):
        y = resample(x[b], bool(params.flip[b]), [int(v) for v in params.box[b]], out_size)
        if m is not None:
            y = y * s + m
        for op in params.ops[b].tolist():
            if op >= 0:
                y = OPS[op](y, float(params.factors[b, op]))
        if bool(params.gray[b]):
            y = np.repeat(gray(y)[None], 3, 0)
        if float(params.blur_sigma[b]) > 0:
            y = blur(y, float(params.blur_sigma[b]))
        if m is not None:
            y = (y - m) / s
        res[b] = y
    return torch.from_numpy(res)


def errors(result, truth):
    """Per image: (max-abs, relative L2) of a float32 result against the float64 truth, two float64 tensors of B values."""
    d = result.detach().cpu().double() - truth
    B = d.shape[0]
    return d.reshape(B, -1).abs().max(1).values, d.reshape(B, -1).norm(dim=1) / truth.reshape(B, -1).norm(dim=1).clamp_min(1e-300)


def dataset_grid(B, H, W):
    """coord (B,H,W,2) of the untransformed dataset grid: channel 0 = linspace(-1,1,H) down the rows."""
    g = torch.stack(torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij"), -1)
    return g[None].expand(B, -1, -1, -1).contiguous()
