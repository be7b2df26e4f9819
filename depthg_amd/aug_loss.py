"""The augmentation-alignment loss term of the training step (src/train_segmentation.py:400-411 under cfg.aug_alignment_weight):
STEGO's regulariser - the code of an augmented view must agree with the code of the original view, sampled where the geometric
augmentation moved each pixel.

    aug_alignment_loss(code, code_aug, coord_aug)     the scalar
        ds   = resize(coord_aug.permute(0,3,1,2), n).permute(0,2,3,1)       src/utils.py:60-61 (bilinear, align_corners=False)
        u    = sample(code, ds)                                             src/modules.py:822-825 (grid_sample of ds.permute(0,2,1,3),
                                                                            border, align_corners=True)
        loss = -mean over (b,i,j) of <norm(u), norm(code_aug)>              src/modules.py:789-790 (F.normalize(dim=1, eps=1e-10))
      code (B,D,h,w) = net(img)[1], code_aug (B,D,n,n) = net(img_aug)[1], coord_aug (B,H,W,2) float32 in [-1, 1]: the dataset's
      meshgrid(linspace(-1,1,H), linspace(-1,1,W)) pushed through the geometric augmentation (src/data.py:1085-1087, 1132-1139),
      channel 0 the row and channel 1 the column coordinate.  On GPU tensors: one fused HIP forward and one HIP backward
      (ops.aug_alignment_forward / aug_alignment_backward, dg_aug.hip) tied together by a torch.autograd.Function; gradients go to
      code and code_aug.  On CPU tensors: the plain differentiable torch chain above, any floating dtype.
    crop_flip_coords(B, H, W, boxes, flips)           a valid coord_aug without torchvision: the grid after an optional horizontal
                                                      flip and a per-image crop resized back to (H, W), what RandomHorizontalFlip +
                                                      RandomResizedCrop do to it (src/train_segmentation.py:602-605)

Two facts about the reference, kept as they are:
  - The two transpositions are reproduced as written: sample() hands grid_sample ds[b,j,i,:] for output (i,j), and grid_sample reads
    channel 0 - the ROW coordinate - as x.  On the untransformed grid the two cancel (u == code when n == h == w).  They do not cancel
    on a mirrored grid: a horizontal flip of the coordinate map samples the vertically mirrored code map.
  - Its line :401 unpacks two values from self.net(img_aug); in training mode this fork's featurizer returns three
    (src/modules.py:128-132), so the branch raises there as written.  The segmenter builds the intent: code_aug = self.net(img_aug)[1].
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops


class _AugAlignment(torch.autograd.Function):
    @staticmethod
    def forward(ctx, code, code_aug, coord_aug):
        loss, ws = ops.aug_alignment_forward(code, code_aug, coord_aug)
        ctx.ws = ws
        ctx.save_for_backward(code, code_aug)
        return loss

    @staticmethod
    @once_differentiable              # (the kernels give the two first derivatives and nothing of higher order)
    def backward(ctx, grad_out):
        code, code_aug = ctx.saved_tensors
        d_code, d_code_aug = ops.aug_alignment_backward(ctx.ws, code, code_aug, grad_out)
        return (d_code if ctx.needs_input_grad[0] else None), (d_code_aug if ctx.needs_input_grad[1] else None), None


def aug_alignment_loss(code, code_aug, coord_aug):
    """-mean <norm(sample(code, resize(coord_aug, n))), norm(code_aug)>, a 0-dim tensor (see the module docstring)."""
    if coord_aug.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("depthg_amd: aug_alignment_loss has no gradient for `coord_aug` (the coordinates are data); detach it")
    if code.dim() != 4 or code_aug.dim() != 4 or coord_aug.dim() != 4:
        raise ValueError(f"depthg_amd: code must be (B, D, h, w), code_aug (B, D, n, n) and coord_aug (B, H, W, 2), got "
                         f"{tuple(code.shape)}, {tuple(code_aug.shape)} and {tuple(coord_aug.shape)}")
    if coord_aug.shape[3] != 2:
        raise ValueError(f"depthg_amd: coord_aug's last axis holds (row, column) coordinates, got {tuple(coord_aug.shape)}")
    if code.shape[0] != code_aug.shape[0] or code.shape[0] != coord_aug.shape[0] or code.shape[1] != code_aug.shape[1]:
        raise ValueError(f"depthg_amd: code {tuple(code.shape)}, code_aug {tuple(code_aug.shape)} and coord_aug {tuple(coord_aug.shape)} "
                         "must share the batch size, the two maps also D")
    if code_aug.shape[2] != code_aug.shape[3]:
        raise ValueError(f"depthg_amd: code_aug must be square - the reference resizes the coordinates to (n, n) and multiplies the "
                         f"maps element by element - got {tuple(code_aug.shape)}")
    if code.is_cuda or code_aug.is_cuda or coord_aug.is_cuda:
        ops._gpu_float32(((code, "code"), (code_aug, "code_aug"), (coord_aug, "coord_aug")),
                         "aug_alignment_loss wants float32 tensors on the GPU, got {name} as {dtype}")
        return _AugAlignment.apply(code, code_aug, coord_aug)
    n = code_aug.shape[2]
    ds = F.interpolate(coord_aug.to(code.dtype).permute(0, 3, 1, 2), (n, n), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    u = F.grid_sample(code, ds.permute(0, 2, 1, 3), padding_mode="border", align_corners=True)
    return -(F.normalize(u, dim=1, eps=1e-10) * F.normalize(code_aug, dim=1, eps=1e-10)).sum(1).mean()


def crop_flip_coords(B, H, W, boxes, flips):
    """coord_aug (B,H,W,2) float32: the dataset's grid (src/data.py:1085-1087: channel 0 = linspace(-1,1,H) down the rows, channel
    1 = linspace(-1,1,W) along the columns) after, per image, an optional horizontal flip and then a crop resized back to (H, W)
    (bilinear, align_corners=False) - RandomHorizontalFlip followed by RandomResizedCrop (src/train_segmentation.py:602-605).
    boxes: B crops (top, left, height, width) in pixels of the flipped grid, fractions allowed, inside the grid; flips: B booleans.
    The full box (0, 0, H, W) without a flip returns the grid itself, bit for bit."""
    if len(boxes) != B or len(flips) != B:
        raise ValueError(f"depthg_amd: crop_flip_coords wants {B} boxes and {B} flips, got {len(boxes)} and {len(flips)}")

    def axis(lin, start, length):
        # the crop's pixels [start, start + length) resized to len(lin) outputs: source (dst + 0.5) * length / size - 0.5, held inside
        # the crop, then the two neighbours of the ramp blended (the ramp is linear: the blend is the resize)
        size = lin.numel()
        src = ((torch.arange(size, dtype=torch.float64) + 0.5) * (float(length) / size) - 0.5).clamp(0.0, max(float(length) - 1.0, 0.0)) + float(start)
        src = src.clamp(0.0, size - 1.0)
        i0 = src.floor().long()
        i1 = (i0 + 1).clamp(max=size - 1)
        f = (src - i0).to(torch.float32)
        return lin[i0] * (1.0 - f) + lin[i1] * f

    out = torch.empty(B, H, W, 2, dtype=torch.float32)
    rows, cols = torch.linspace(-1, 1, H), torch.linspace(-1, 1, W)
    for b, ((top, left, bh, bw), flip) in enumerate(zip(boxes, flips)):
        if not (bh > 0 and bw > 0 and top >= 0 and left >= 0 and top + bh <= H and left + bw <= W):
            raise ValueError(f"depthg_amd: crop box {(top, left, bh, bw)} of image {b} leaves the {H}x{W} grid")
        out[b, :, :, 0] = axis(rows, top, bh)[:, None]
        out[b, :, :, 1] = axis(cols.flip(0) if flip else cols, left, bw)[None, :]
    return out
