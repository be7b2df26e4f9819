"""The two probes of the training step (src/train_segmentation.py:421-444, src/modules.py:647-675 with alpha None) restated in
float64 with analytic gradients - the truth the tests of head.fused_probe_losses measure against - the same chain in the inputs'
dtype for autograd (the yardstick), and the makers of the inputs both share.  The product does not import this module.

    low  = W c + b                                  (B, n_lin, h, w)   the linear probe, a 1 x 1 convolution
    up   = Ry low Rx^T                              (B, n_lin, H, W)   F.interpolate(bilinear, align_corners=False) as two tap matrices
    linear_loss  = mean over {0 <= label < n_lin} of -log softmax(up)[label]
    d up = g_lin (softmax(up) - one_hot(label)) mask / count,   d low = Ry^T d up Rx,   d W = sum d low c^T,   d b = sum d low
    cluster_loss = -mean_{b,p} max_j <nc_j, nx_{b,p}>,          nc = normalize(clusters), nx = normalize(c)
    g_j = -(g_clu / (B h w)) sum over {p : arg-max = j} of nx_p,   d clusters_j = (g_j - nc_j <nc_j, g_j>) / |clusters_j|
The code is detached in the reference (:421): it receives no gradient.

MARGIN INPUTS: the arg-max is a discrete switch - a float32 route whose rounding picks another centre at one position computes another
function there.  margin_inputs() redraws every position whose two largest cosine similarities lie closer than GAP in float64, and
asserts the gap, so that no float32 route can flip a winner (the similarities are O(1): float32 rounding moves them by ~1e-6).
"""
import functools
import math

import torch
import torch.nn.functional as F

GAP = 1e-3
# name: (B, D, n_lin, n_clu, (h, w), (H, W)) - the smallest shapes at which each part of the kernels can go wrong
SHAPES = {
    "tiny": (2, 8, 3, 5, (4, 4), (8, 8)),                   # everything smaller than one tile
    "ragged": (3, 70, 27, 30, (5, 7), (20, 28)),            # integer ratio, n_clu != n_lin, B h w no multiple of 64
    "ratios": (2, 16, 4, 4, (7, 7), (20, 33)),              # non-integer ratios, W over several taps per column
    "limits": (1, 128, 64, 64, (3, 3), (5, 4)),             # D = 128, n_lin = n_clu = 64
    "train": (2, 70, 27, 27, (28, 28), (224, 224)),         # the training shape: 13 position chunks per image, 8 label rows per feature row
}
UPSTREAM = ((1.0, 1.0), (0.7, -1.3))
GRADS = ("d_weight", "d_bias", "d_clusters")


def spacing32(x):
    """One float32 spacing at the magnitude of x."""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x != 0 else 2.0 ** -149


def resize_matrix(out, inn):
    """(out, inn) float64: the tap matrix of F.interpolate(mode="bilinear", align_corners=False) along one axis."""
    M = torch.zeros(out, inn, dtype=torch.float64)
    for i in range(out):
        src = max((i + 0.5) * inn / out - 0.5, 0.0)
        i0 = min(int(src), inn - 1)
        i1 = min(i0 + 1, inn - 1)
        M[i, i0] += 1.0 - (src - i0)
        M[i, i1] += src - i0
    return M


def top_two_gap(code, clusters):
    """(B, h, w) float64: the distance of the two largest cosine similarities at every position."""
    inner = torch.einsum("bchw,nc->bnhw", F.normalize(code.double(), dim=1), F.normalize(clusters.double(), dim=1))
    top = inner.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def margin_inputs(B, D, m, hw, gen):
    """code (B, D, h, w), clusters (m, D) float32 whose arg-max no float32 route can flip: every position's gap is >= GAP in float64."""
    code, clusters = torch.randn(B, D, *hw, generator=gen), torch.randn(m, D, generator=gen)
    for _ in range(200):
        close = top_two_gap(code, clusters) < GAP
        if not bool(close.any()):
            break
        fresh = torch.randn(B, D, *hw, generator=gen)
        code = torch.where(close[:, None], fresh, code)
    assert float(top_two_gap(code, clusters).min()) >= GAP, "margin_inputs: a position's two best centres stayed closer than GAP"
    return code, clusters


def make_label(B, n, HW, gen):
    """int64 (B, H, W): classes in [0, n), with -1, values >= n, one row of image 0 entirely unlabelled and - when there is more than
    one image - the LAST image without any labelled pixel."""
    H, W = HW
    lab = torch.randint(0, n, (B, H, W), generator=gen)
    u = torch.rand(B, H, W, generator=gen)
    lab[u < 0.15] = -1
    lab[(u >= 0.15) & (u < 0.22)] = n
    lab[(u >= 0.22) & (u < 0.25)] = 255
    lab[0, H // 2] = -1
    if B > 1:
        lab[B - 1] = -1
    return lab


@functools.lru_cache(maxsize=None)
def operands(shape):
    """(code, label, weight (n_lin, D, 1, 1), bias, clusters) of a case, float32 / int64, seeded by the case's position."""
    B, D, n, m, hw, HW = SHAPES[shape]
    gen = torch.Generator().manual_seed(4100 + list(SHAPES).index(shape))
    code, clusters = margin_inputs(B, D, m, hw, gen)
    bound = 1.0 / math.sqrt(D)                              # nn.Conv2d's default initialisation, scaled up to logits of O(1)
    weight = (torch.rand(n, D, 1, 1, generator=gen) * 2 - 1) * bound * 4
    bias = (torch.rand(n, generator=gen) * 2 - 1) * bound
    return code, make_label(B, n, HW, gen), weight, bias, clusters


def chain(code, label, weight, bias, clusters, g_lin=1.0, g_clu=1.0):
    """dict(linear_loss, cluster_loss, count, d_weight (n_lin, D), d_bias, d_clusters, arg (B, h, w)), float64, from the formulas above."""
    code, bias, clusters = code.double(), bias.double(), clusters.double()
    B, D, h, w = code.shape
    n = weight.shape[0]
    W2 = weight.double().reshape(n, D)
    H, Wd = label.shape[-2:]
    label = label.reshape(B, H, Wd)
    Ry, Rx = resize_matrix(H, h), resize_matrix(Wd, w)
    low = torch.einsum("nd,bdhw->bnhw", W2, code) + bias[None, :, None, None]
    up = torch.einsum("Yy,bnyx,Xx->bnYX", Ry, low, Rx)
    mask = (label >= 0) & (label < n)
    count = int(mask.sum())
    logp = torch.log_softmax(up, dim=1)
    safe = label.clamp(0, n - 1)
    picked = logp.gather(1, safe[:, None])[:, 0]
    linear_loss = float(-(picked * mask).sum() / count) if count else float("nan")
    d_up = (logp.exp() - F.one_hot(safe, n).permute(0, 3, 1, 2)) * mask[:, None] * (g_lin / count if count else float("nan"))
    d_low = torch.einsum("Yy,bnYX,Xx->bnyx", Ry, d_up, Rx)
    out = {"linear_loss": linear_loss, "count": count, "d_weight": torch.einsum("bnyx,bdyx->nd", d_low, code), "d_bias": d_low.sum((0, 2, 3))}
    norm_c = clusters.norm(dim=1, keepdim=True).clamp_min(1e-12)
    nc, nx = clusters / norm_c, F.normalize(code, dim=1)
    inner = torch.einsum("bchw,nc->bnhw", nx, nc)
    best, arg = inner.max(dim=1)
    g = torch.einsum("bmhw,bdhw->md", F.one_hot(arg, clusters.shape[0]).permute(0, 3, 1, 2).double(), nx) * (-g_clu / (B * h * w))
    out.update({"cluster_loss": float(-best.mean()), "arg": arg, "d_clusters": (g - nc * (nc * g).sum(1, keepdim=True)) / norm_c})
    return out


@functools.lru_cache(maxsize=None)
def truth(shape, upstream=(1.0, 1.0)):
    return chain(*operands(shape), *upstream)


def torch_chain(code, label, weight, bias, clusters):
    """(linear_loss, cluster_loss) as the reference forms them - conv2d, interpolate, three masks, CrossEntropyLoss; ClusterLookup
    with alpha None - in the inputs' dtype, for autograd: the float32 yardstick."""
    n = weight.shape[0]
    logits = F.interpolate(F.conv2d(code, weight, bias), label.shape[-2:], mode="bilinear", align_corners=False)
    flat, lab = logits.permute(0, 2, 3, 1).reshape(-1, n), label.reshape(-1)
    mask = (lab >= 0) & (lab < n)
    linear_loss = F.cross_entropy(flat[mask], lab[mask])
    inner = torch.einsum("bchw,nc->bnhw", F.normalize(code, dim=1), F.normalize(clusters, dim=1))
    probs = F.one_hot(torch.argmax(inner, dim=1), clusters.shape[0]).permute(0, 3, 1, 2).to(inner.dtype)
    return linear_loss, -(probs * inner).sum(1).mean()


def run(fn, ops, upstream, dev):
    """(linear_loss, cluster_loss, d_weight (n, D), d_bias, d_clusters) of `fn` on `dev` under the upstream scalars, as float64 on the CPU."""
    code, label, weight, bias, clusters = ops
    w, b, c = (t.detach().clone().to(dev).requires_grad_(True) for t in (weight, bias, clusters))
    lin, clu = fn(code.to(dev), label.to(dev), w, b, c)
    (upstream[0] * lin + upstream[1] * clu).backward()
    return (float(lin.detach().double()), float(clu.detach().double()), w.grad.double().cpu().reshape(w.shape[0], -1), b.grad.double().cpu(),
            c.grad.double().cpu())


def figures(got, t):
    """The error figures of the loss terms' tests: a loss's absolute error floored at one float32 spacing of the loss (no route can
    return a better scalar than the format holds), a gradient's relative L2 error."""
    rel = lambda g, want: float((g - want).norm() / want.norm())
    return {"linear_loss": max(abs(got[0] - t["linear_loss"]), spacing32(t["linear_loss"])),
            "cluster_loss": max(abs(got[1] - t["cluster_loss"]), spacing32(t["cluster_loss"])),
            **{k: rel(g, t[k]) for g, k in zip(got[2:], GRADS)}}
