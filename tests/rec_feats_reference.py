"""d loss / d feats of the reconstruction term (rec_loss.reconstruction_loss(feats_grad=True), dg_rec_feats_backward) in float64 - the
truth tests/test_rec_feats_cpu.py and tests/test_gpu_rec_feats.py measure against - on the shapes and input makers of
tests/rec_loss_reference.py.  With that module's y, f, ny, nf, s, a:

    d f = a y + b' f,   a = -(G/N) / (ny nf),   b' = (G/N) s / nf^2 where |f| > eps else 0,   ny = max(|y|, eps), nf = max(|f|, eps)

(dy = a f + b y with the roles of y and f exchanged; the `else 0` is F.normalize under autograd, as for b).  Under Dropout2d keep
flags f = raw (keep scale) and the gradient is the un-dropped map's: d raw = d f (keep scale), a dropped channel exactly 0.

One kind more than rec_loss_reference.KINDS: "small_f" - the "random" inputs with all channels of feats zero at a few positions, so
that |f| = 0 < eps there: b' = 0, nf = eps, and d f = a y is the partner's unit vector over eps (about 1e10 / N, finite).
"""
import functools

import torch
import torch.nn.functional as F

import rec_loss_reference as R

EPS = R.EPS
SHAPES = {k: v for k, v in R.SHAPES.items() if k != "wraps"}        # (more loss partials than one reduction holds: nothing d feats reaches)
KINDS = R.KINDS + ("small_f",)
CASES = [(shape, kind) for shape, kind in R.CASES if shape in SHAPES] + [("tiny", "small_f"), ("ragged", "small_f"), ("head", "small_f")]


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    """rec_loss_reference.inputs, and for "small_f" its "random" inputs with feats zeroed at three positions (two in the first image,
    the last position of the last image).  Shared by the tests, never modified."""
    if kind != "small_f":
        return R.inputs(shape, kind)
    i = dict(R.inputs(shape, "random"))
    B, _, _, (h, w) = R.SHAPES[shape]
    raw = i["raw"].clone()
    for b, y, x in ((0, 0, 0), (0, h // 2, w - 1), (B - 1, h - 1, w - 1)):
        raw[b, :, y, x] = 0
    i["raw"] = i["feats"] = raw
    return i


def d_feats(code, feats, weight, bias, keep=None, scale=1.0, grad_out=1.0):
    """The formula above in float64: `feats` is what the term sees (the dropped map when keep is given); returns the gradient of the
    un-dropped map then, else of feats."""
    code, feats, bias = code.double(), feats.double(), bias.double()
    C, D = feats.shape[1], code.shape[1]
    y = F.conv2d(code, weight.double().reshape(C, D, 1, 1), bias)
    ny, nf = y.square().sum(1).sqrt(), feats.square().sum(1).sqrt()
    nyc, nfc = ny.clamp(min=EPS), nf.clamp(min=EPS)
    s = (y * feats).sum(1) / (nyc * nfc)
    g = grad_out / s.numel()
    a = -g / (nyc * nfc)
    bf = torch.where(nf > EPS, g * s / nfc.square(), torch.zeros_like(s))
    df = a[:, None] * y + bf[:, None] * feats
    if keep is not None:
        df = df * (keep.double() * scale)[:, :, None, None]
    return df


@functools.lru_cache(maxsize=None)
def truth(shape, kind):
    """d_feats of inputs(shape, kind), once per case - shared by the tests, never modified."""
    i = inputs(shape, kind)
    return d_feats(i["code"], i["feats"], i["weight"], i["bias"], i["keep"], i["scale"])


def torch_d_feats(shape, kind, dtype=torch.float64, device="cpu"):
    """Autograd of rec_loss_reference.torch_chain with respect to the (un-dropped) feature map, in `dtype` on `device`: the check of
    the formula (float64) and the GPU tests' yardstick (float32)."""
    i = inputs(shape, kind)
    code, weight, bias, raw = (i[k].to(device=device, dtype=dtype) for k in ("code", "weight", "bias", "raw"))
    raw.requires_grad_(True)
    feats = raw if i["keep"] is None else raw * (i["keep"].to(device=device, dtype=dtype) * i["scale"])[:, :, None, None]
    R.torch_chain(code, feats, weight, bias).backward()
    return raw.grad


def check_formula(shape, kind):
    """The float64 restatement against float64 autograd: relative L2 (absolute, for the vanishing gradient of `aligned`)."""
    want, got = torch_d_feats(shape, kind), truth(shape, kind)
    if kind == "aligned":
        return float((got - want).abs().max())
    return float((got - want).norm() / want.norm())
