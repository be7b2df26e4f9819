"""Dense-CRF refinement (src/crf.py) on the GPU: the reference runs pydensecrf's DenseCRF2D per image on the host; here mean-field
inference runs in HIP (ops.dense_crf -> dg_dense_crf, depthg_amd/csrc/dg_crf.hip), whole batches at a time.

    dense_crf(image_tensor, output_logits)   src/crf.py:22-49 for one image: (C,H,W) fp32 on the GPU
    batched_crf(img_tensor, prob_tensor)     the drop-in for batched_crf of src/eval_segmentation.py:55-60 (without the pool):
                                             (B,C,H,W) fp32 on the GPU

The colour image is UnNormalize then mul(255).byte() as the reference's to_pil_image(unnorm(...)) computes it; values outside
[0, 255], which the reference leaves to an undefined byte conversion, are clamped.  Unlike the reference, the results stay on the GPU.
"""
import torch

from . import ops

MAX_ITER = 10
POS_W = 3
POS_XY_STD = 1
Bi_W = 4
Bi_XY_STD = 67
Bi_RGB_STD = 3


def _run(img, logits):
    H, W = img.shape[-2:]
    U = ops.crf_unary(logits, H, W)
    q, _ = ops.dense_crf(img, U, n_iter=MAX_ITER, pos_w=POS_W, pos_xy_std=POS_XY_STD, bi_w=Bi_W, bi_xy_std=Bi_XY_STD,
                         bi_rgb_std=Bi_RGB_STD)
    return q


def dense_crf(image_tensor: torch.Tensor, output_logits: torch.Tensor) -> torch.Tensor:
    """image_tensor (3,H,W) normalised, output_logits (C,h,w) (resized to (H,W), bilinear, align_corners=False); both on the GPU.
    Returns Q (C,H,W) fp32."""
    if image_tensor.dim() != 3 or output_logits.dim() != 3:
        raise ValueError(f"depthg_amd: dense_crf takes (3,H,W) and (C,h,w), got {tuple(image_tensor.shape)} and "
                         f"{tuple(output_logits.shape)}")
    with torch.no_grad():
        return _run(image_tensor.unsqueeze(0), output_logits.unsqueeze(0))[0]


def batched_crf(img_tensor: torch.Tensor, prob_tensor: torch.Tensor) -> torch.Tensor:
    """img_tensor (B,3,H,W) normalised, prob_tensor (B,C,h,w) logits (or log-probabilities); both on the GPU.  Returns (B,C,H,W)."""
    if img_tensor.dim() != 4 or prob_tensor.dim() != 4 or img_tensor.shape[0] != prob_tensor.shape[0]:
        raise ValueError(f"depthg_amd: batched_crf takes (B,3,H,W) and (B,C,h,w), got {tuple(img_tensor.shape)} and "
                         f"{tuple(prob_tensor.shape)}")
    with torch.no_grad():
        return _run(img_tensor, prob_tensor)
