"""The reconstruction term (src/train_segmentation.py:391-398) in float64 torch with analytic gradients - the truth the CPU and GPU
tests measure against - and the input makers both share.

    y    = conv2d(code, W, b)                              the decoder, nn.Conv2d(dim, n_feats, (1, 1)) (src/train_segmentation.py:115)
    s    = <normalize(y), normalize(f)>,  loss = -mean s   F.normalize(dim=1, eps=1e-10) (src/modules.py:789-790)
    dy   = a f + b y,  a = -(G/N) / (ny nf),  b = (G/N) s / ny^2 where |y| > eps else 0,  ny = max(|y|, eps), nf = max(|f|, eps)
    d code = W^T dy,  d W = sum_p dy c_p^T,  d b = sum_p dy
(the `else 0` is F.normalize under autograd: clamp_min passes no gradient below eps).  chain() forms the loss through F.conv2d and
F.normalize and the gradients from the formulas; torch_chain() is the same chain for autograd, in the inputs' dtype.
"""
import functools
import math

import torch
import torch.nn.functional as F

EPS = 1e-10
# name: (B, D, C, (h, w)) - the smallest shapes that reach each tail of the kernels
SHAPES = {
    "tiny": (2, 3, 5, (2, 2)),            # everything smaller than one chunk or wave
    "ragged": (2, 70, 100, (5, 7)),       # C and h w multiples of nothing
    "head": (2, 70, 384, (8, 8)),         # the training widths
    "wide": (1, 27, 1024, (4, 4)),        # many channel chunks; dim = n_classes
    "tall": (3, 128, 64, (9, 9)),         # the D limit
    "many": (2, 16, 32, (40, 40)),        # several position blocks per image, more than one partial in every reduction
    "wraps": (5, 3, 5, (58, 58)),         # 5 x 53 = 265 tiles: more partials than k_loss_reduce has threads (sorts last: inputs() seeds by position)
}
KINDS = ("random", "scaled", "dropped", "aligned")
CASES = [(shape, "random") for shape in SHAPES] + [("ragged", "scaled"), ("head", "scaled"), ("ragged", "dropped"), ("head", "dropped"),
                                                   ("many", "dropped"), ("tiny", "aligned"), ("head", "aligned")]


def chain(code, feats, weight, bias, grad_out=1.0):
    """dict(loss, d_code, d_weight (C,D), d_bias, s (B,h,w), norm_y, norm_f, mean_abs_s), float64."""
    code, feats, bias = code.double(), feats.double(), bias.double()
    C, D = feats.shape[1], code.shape[1]
    weight = weight.double().reshape(C, D)
    y = F.conv2d(code, weight.view(C, D, 1, 1), bias)
    ny, nf = y.square().sum(1).sqrt(), feats.square().sum(1).sqrt()
    s = (F.normalize(y, dim=1, eps=EPS) * F.normalize(feats, dim=1, eps=EPS)).sum(1)
    g = grad_out / s.numel()
    nyc, nfc = ny.clamp(min=EPS), nf.clamp(min=EPS)
    a = -g / (nyc * nfc)
    b = torch.where(ny > EPS, g * s / nyc.square(), torch.zeros_like(s))
    dy = a[:, None] * feats + b[:, None] * y
    return {"loss": float(-s.mean()), "d_code": torch.einsum("cd,bchw->bdhw", weight, dy), "d_weight": torch.einsum("bchw,bdhw->cd", dy, code),
            "d_bias": dy.sum((0, 2, 3)), "s": s, "norm_y": ny, "norm_f": nf, "mean_abs_s": float(s.abs().mean())}


def torch_chain(code, feats, weight, bias):
    """The reference's chain in torch, differentiable, in the tensors' dtype and on their device."""
    C, D = feats.shape[1], code.shape[1]
    rec_feats = F.conv2d(code, weight.reshape(C, D, 1, 1), bias)
    return -(F.normalize(rec_feats, dim=1, eps=1e-10) * F.normalize(feats, dim=1, eps=1e-10)).sum(1).mean()


def spacing32(x):
    """One float32 spacing at the magnitude of x."""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x != 0 else 2.0 ** -149


def decoder_init(C, D, gen):
    """nn.Conv2d(D, C, (1, 1))'s default initialisation: weight and bias uniform in +-1/sqrt(fan_in), from `gen`."""
    bound = 1.0 / math.sqrt(D)
    weight = (torch.rand(C, D, 1, 1, generator=gen) * 2 - 1) * bound
    return weight, (torch.rand(C, generator=gen) * 2 - 1) * bound


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    """dict(code, feats, weight (C,D,1,1), bias, keep, scale, raw) on the CPU, float32.  feats is what the term sees; for `dropped`
    raw is the un-dropped map and feats = raw * (keep * scale) - ops.DeferredDropout(raw, keep, scale).materialize() - else keep is
    None and raw is feats.  Shared by the tests, never modified."""
    B, D, C, (h, w) = SHAPES[shape]
    gen = torch.Generator().manual_seed(2000 + 10 * sorted(SHAPES).index(shape) + KINDS.index(kind))
    code = torch.randn(B, D, h, w, generator=gen) + 0.6
    weight, bias = decoder_init(C, D, gen)
    raw = torch.randn(B, C, h, w, generator=gen) + 0.3
    keep, scale = None, 1.0
    if kind == "scaled":
        raw, code = raw * 1e3, code * 1e-3
    elif kind == "aligned":                # s = 1 everywhere and the true gradient vanishes
        raw = F.conv2d(code, weight, bias)
    feats = raw
    if kind == "dropped":                  # Dropout2d with p = 0.5
        keep, scale = torch.empty(B, C).bernoulli_(0.5, generator=gen), 2.0
        feats = raw * (keep * scale)[:, :, None, None]
    return {"code": code, "feats": feats, "weight": weight, "bias": bias, "keep": keep, "scale": scale, "raw": raw}


def operands(shape, kind):
    i = inputs(shape, kind)
    return i["code"], i["feats"], i["weight"], i["bias"]


@functools.lru_cache(maxsize=None)
def truth(shape, kind):
    """chain() of inputs(shape, kind), once per case - shared by the tests, never modified."""
    return chain(*operands(shape, kind))
