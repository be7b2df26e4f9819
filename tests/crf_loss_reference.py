"""A float64 restatement of the contrastive CRF term of the training step, written from its formulas for the tests: the bilinear resize
(align_corners=False, no antialiasing), the channel normalisation with its eps clamp, the pick of n sample positions shared by the
batch, the pairwise similarity kernel and the mean.  torch float64 throughout, so that autograd gives the gradient to the code map.
Imported by the tests the way conftest is.

    K_ac = w1 exp(-|p_a - p_c|^2 / (2 alpha) - |g_a - g_c|^2 / (2 beta)) + w2 exp(-|p_a - p_c|^2 / (2 gamma)) - shift
    out  = -(S_a . S_c) K_ac          (B,n,n)
"""
import torch

DEFAULT_SET = dict(alpha=.5, beta=.15, gamma=.05, w1=10.0, w2=3.0, shift=0.0)       # nearly diagonal
DENSE_SET = dict(alpha=200.0, beta=.5, gamma=50.0, w1=10.0, w2=3.0, shift=.3)       # off-diagonal terms carry the loss


def _axis_taps(n_in, n_out, dtype):
    """Per output index: the two source indices and the weight of the second (source coordinate max((dst + 0.5) in / out - 0.5, 0))."""
    dst = torch.arange(n_out, dtype=dtype)
    src = ((dst + 0.5) * (n_in / n_out) - 0.5).clamp(min=0)
    i0 = src.floor().clamp(max=n_in - 1)
    lam = src - i0
    i0 = i0.long()
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, lam


def resize(x, size):
    """(B,C,h,w) -> (B,C,size,size), bilinear."""
    _, _, h, w = x.shape
    y0, y1, ly = _axis_taps(h, size, x.dtype)
    x0, x1, lx = _axis_taps(w, size, x.dtype)
    rows = x[:, :, y0, :] * (1 - ly)[None, None, :, None] + x[:, :, y1, :] * ly[None, None, :, None]
    return rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx


def normalise(x, eps=1e-10):
    """x / max(|x|, eps) over the channels."""
    return x / x.square().sum(1, keepdim=True).sqrt().clamp(min=eps)


def kernel_matrix(guidance, coords, alpha, beta, gamma, w1, w2, shift):
    """guidance (B,3,s,s), coords (2,n) integer (rows, columns) -> K, (B,n,n)."""
    ys, xs = coords[0].long(), coords[1].long()
    p = torch.stack([ys, xs], 1).to(guidance.dtype)                     # (n,2)
    dp = (p[:, None, :] - p[None, :, :]).square().sum(-1)               # (n,n)
    g = guidance[:, :, ys, xs].permute(0, 2, 1)                         # (B,n,3)
    dg = (g[:, :, None, :] - g[:, None, :, :]).square().sum(-1)         # (B,n,n)
    return w1 * torch.exp(-dp / (2 * alpha) - dg / (2 * beta)) + w2 * torch.exp(-dp / (2 * gamma)) - shift


def pair_tensor(guidance, clusters, coords, alpha, beta, gamma, w1, w2, shift):
    """guidance (B,3,s,s), clusters (B,D,s,s), coords (2,n) integer (rows, columns) -> -(sims * K), (B,n,n)."""
    ys, xs = coords[0].long(), coords[1].long()
    K = kernel_matrix(guidance, coords, alpha, beta, gamma, w1, w2, shift)
    S = clusters[:, :, ys, xs].permute(0, 2, 1)                         # (B,n,D)
    return -(S @ S.transpose(1, 2)) * K


def chain(img, code, coords, size, scalars):
    """The whole term on float64 copies of the inputs: (loss, d loss / d code, mean |sims * K|, S (B,n,D), g (B,n,3))."""
    img64 = img.detach().double().cpu()
    code64 = code.detach().double().cpu().requires_grad_(True)
    coords = coords.cpu()
    guidance, clusters = resize(img64, size), normalise(resize(code64, size))
    out = pair_tensor(guidance, clusters, coords, **scalars)
    loss = out.mean()
    grad, = torch.autograd.grad(loss, code64)
    ys, xs = coords[0].long(), coords[1].long()
    return (float(loss.detach()), grad, float(out.detach().abs().mean()), clusters.detach()[:, :, ys, xs].permute(0, 2, 1),
            guidance[:, :, ys, xs].permute(0, 2, 1))


def gradient_scale(img, code, coords, size, scalars):
    """What an element of d loss / d code could reach if nothing cancelled: with dS_a = -(2 / (B n^2)) sum_c K_ac S_c, |S_c| = 1, and
    the adjoint of the normalisation dividing by |x_a|, at most (2 / (B n^2)) sum_a (sum_c |K_ac|) / |x_a| lands on one pixel (the
    resize's tap weights are <= 1).  The largest over the images, float64."""
    img64, code64, coords = img.detach().double().cpu(), code.detach().double().cpu(), coords.cpu()
    ys, xs = coords[0].long(), coords[1].long()
    K = kernel_matrix(resize(img64, size), coords, **scalars)                      # (B,n,n)
    norms = resize(code64, size).square().sum(1).sqrt()[:, ys, xs]                 # (B,n)
    B, n = norms.shape
    return float((K.abs().sum(2) / norms).sum(1).max()) * 2.0 / (B * n * n)
