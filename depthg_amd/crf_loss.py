"""ContrastiveCRFLoss (src/modules.py:1510-1542; built at src/train_segmentation.py:128-129, used at :413-419 under cfg.crf_weight).

Two routes over one set of scalars:
    forward(guidance, clusters, coords=None)       the reference's contract in plain torch, CPU or GPU: -(sims * K) as (B,n,n).  For
                                                   callers who want the tensor; not the hot path.
    mean_loss(img, code, size=56, coords=None)     what the training step needs, `crf_loss_fn(resize(img, size),
                                                   norm(resize(code, size))).mean()`, as one fused HIP forward (ops.crf_loss_forward:
                                                   the maps are resized at the n sampled positions only and K is formed on the fly) and
                                                   one HIP backward (ops.crf_loss_backward), tied together by a torch.autograd.Function.
                                                   The gradient goes to `code` only.
Both draw their sample coordinates the way the reference does when none are given: torch.randint(0, h, [1, n]) for the rows, then
torch.randint(0, w, [1, n]) for the columns, on the maps' device.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops


def draw_coords(h, w, n, device):
    """(2, n) int64 sample positions shared by the batch: n rows in [0, h), then n columns in [0, w).  The order and the shapes of
    the two draws are the reference's (src/modules.py:1529-1531), so that a seeded run picks the reference's samples."""
    rows = torch.randint(0, h, size=[1, n], device=device)
    cols = torch.randint(0, w, size=[1, n], device=device)
    return torch.cat([rows, cols], 0)


class _MeanCRFLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, code, img, coords, size, scalars):
        loss, ws = ops.crf_loss_forward(code, img, coords, size, *scalars)
        ctx.ws, ctx.coords, ctx.size, ctx.shape_code = ws, coords, size, tuple(code.shape)
        return loss

    @staticmethod
    @once_differentiable              # (the kernels give d loss / d code and nothing of higher order: a double backward is refused)
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        return ops.crf_loss_backward(ctx.ws, ctx.coords, ctx.shape_code, ctx.size, grad_out), None, None, None, None


class ContrastiveCRFLoss(nn.Module):
    """The seven constructor arguments and their attribute names are the reference's (src/modules.py:1512-1520)."""

    def __init__(self, n_samples, alpha, beta, gamma, w1, w2, shift):
        super().__init__()
        self.n_samples = n_samples
        self.alpha, self.beta, self.gamma, self.w1, self.w2, self.shift = alpha, beta, gamma, w1, w2, shift

    def _scalars(self):
        return (self.alpha, self.beta, self.gamma, self.w1, self.w2, self.shift)

    def forward(self, guidance, clusters, coords=None):
        """guidance (B,3,h,w), clusters (B,D,h,w) of equal spatial size -> -(sims * K), (B,n,n), with
            K_ac = w1 exp(-|p_a - p_c|^2 / (2 alpha) - |g_a - g_c|^2 / (2 beta)) + w2 exp(-|p_a - p_c|^2 / (2 gamma)) - shift
        over n sample positions p shared by the batch, g the guidance and sims the dot products of the clusters there.
        coords: (2,n) integer rows / columns; drawn by draw_coords when None."""
        if guidance.dim() != 4 or clusters.dim() != 4 or guidance.shape[0] != clusters.shape[0] or guidance.shape[2:] != clusters.shape[2:]:
            raise ValueError(f"depthg_amd: guidance {tuple(guidance.shape)} and clusters {tuple(clusters.shape)} must share batch and "
                             "spatial size")
        dev, dt = clusters.device, clusters.dtype
        if coords is None:
            coords = draw_coords(guidance.shape[2], guidance.shape[3], self.n_samples, dev)
        rows, cols = coords[0].to(dev, torch.long), coords[1].to(dev, torch.long)
        # squared distances between the samples: positions (small integers: exact in any float type), then colours, one channel
        # after the other
        pos = torch.stack([rows, cols], dim=1).to(dt)                                  # (n,2)
        step = pos[:, None, :] - pos[None, :, :]
        dist_pos = step[..., 0] ** 2 + step[..., 1] ** 2                               # (n,n)
        colour = guidance[:, :, rows, cols].transpose(1, 2)                            # (B,n,3)
        dc = colour[:, :, None, :] - colour[:, None, :, :]
        dist_col = dc[..., 0] ** 2 + dc[..., 1] ** 2 + dc[..., 2] ** 2                 # (B,n,n)
        near = torch.exp(-(dist_pos / (2 * self.alpha) + dist_col / (2 * self.beta)))  # appearance and position
        far = torch.exp(-dist_pos / (2 * self.gamma))                                  # position alone
        kernel = self.w1 * near + self.w2 * far - self.shift
        picked = clusters[:, :, rows, cols]                                            # (B,D,n)
        sims = picked.transpose(1, 2) @ picked                                         # (B,n,n)
        return -(kernel * sims)

    def mean_loss(self, img, code, size=56, coords=None):
        """The scalar `self(resize(img, size), norm(resize(code, size))).mean()` (src/train_segmentation.py:414-417) on the fused HIP
        route.  img (B,3,H,W), code (B,D,h,w) on the GPU; coords (2,n) on the size x size grid, drawn as in forward() when None."""
        if img.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("depthg_amd: ContrastiveCRFLoss.mean_loss has no gradient for `img` (the guidance is the input image); "
                               "detach it")
        # (img takes no gradient: ops.crf_loss_forward may cast it)
        ops._gpu_float32(((code, "code"),), "ContrastiveCRFLoss.mean_loss wants a float32 code map, got {dtype}", also_gpu=((img, "img"),))
        size = int(size)
        if coords is None:
            coords = draw_coords(size, size, self.n_samples, code.device)
        return _MeanCRFLoss.apply(code, img, coords, size, self._scalars())
