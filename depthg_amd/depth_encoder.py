"""The depth encoder of DinoFeaturizerWithDepth (src/modules.py:497-506 `depth_downscaling`, :557 its call, :562-563 the "sum"
guidance's add) as one fused HIP forward and one fused HIP backward.

    depth_encoder(depth, stack, residual=None)      (B, C, h, w)
        stack(depth) [+ residual]
      depth (B, 1, 8h, 8w) or (B, 8h, 8w); stack the three-stage nn.Sequential of featurizer.make_depth_downscaling (n_feats == 384):
          Conv2d(1,64,2,2), LayerNorm2d(64), GELU, Conv2d(64,128,2,2), LayerNorm2d(128), GELU, Conv2d(128,C,2,2)
      - the five-stage form is refused; residual: a (B, C, h, w) map without grad (the frozen backbone's features), added in the
      kernel's epilogue.  On GPU tensors: ops.depth_encoder_forward / depth_encoder_backward (dg_depth_enc.hip) tied together by a
      torch.autograd.Function; gradients go to the stack's ten parameters - no activation map of stage 1 or 2 is written in either
      direction - and a depth map that requires grad is refused (the kernels have no d depth).  On CPU tensors: the plain torch
      modules, bit for bit what `stack(depth) + residual` gives.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops


def stack_parameters(stack):
    """The ten parameters of the three-stage stack in module order (w1, b1, gamma1, beta1, w2, b2, gamma2, beta2, w3, b3); a
    ValueError for anything else (the five-stage stack of n_feats != 384 among them)."""
    from .featurizer import LayerNorm2d
    kinds = (nn.Conv2d, LayerNorm2d, nn.GELU, nn.Conv2d, LayerNorm2d, nn.GELU, nn.Conv2d)
    mods = list(stack) if isinstance(stack, nn.Sequential) else []
    ok = len(mods) == len(kinds) and all(isinstance(m, k) for m, k in zip(mods, kinds))
    if ok:
        convs, norms = (mods[0], mods[3], mods[6]), (mods[1], mods[4])
        ok = all(c.kernel_size == (2, 2) and c.stride == (2, 2) and c.padding == (0, 0) and c.dilation == (1, 1) and c.groups == 1 and
                 c.bias is not None for c in convs)
        ok = ok and (convs[0].in_channels, convs[0].out_channels, convs[1].out_channels) == (1, 64, 128)
        ok = ok and all(n.eps == 1e-6 for n in norms) and all(getattr(m, "approximate", "none") == "none" for m in (mods[2], mods[5]))
    if not ok:
        raise ValueError("depthg_amd: depth_encoder takes the three-stage stack of make_depth_downscaling(384) - Conv2d(1,64,2,2), "
                         "LayerNorm2d(64), GELU, Conv2d(64,128,2,2), LayerNorm2d(128), GELU, Conv2d(128,C,2,2); the five-stage stack "
                         "(n_feats != 384) stays on the torch route")
    return [mods[0].weight, mods[0].bias, mods[1].weight, mods[1].bias, mods[3].weight, mods[3].bias, mods[4].weight, mods[4].bias,
            mods[6].weight, mods[6].bias]


class _DepthEncoder(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, residual, *params):
        # contiguous float32 once: both directions read this depth map, and a strided one is copied here and nowhere else
        d, p, res, (B, C, h, w) = ops._depth_encoder_operands(depth, params, residual, "residual")
        ctx.save_for_backward(d, *params)
        return ops.depth_encoder_forward(d, p, res)

    @staticmethod
    @once_differentiable              # (the kernels give the ten first derivatives and nothing of higher order)
    def backward(ctx, grad_out):
        d, *params = ctx.saved_tensors
        grads = ops.depth_encoder_backward(d, params, grad_out)
        need = ctx.needs_input_grad
        return (None, None, *[g if need[2 + k] else None for k, g in enumerate(grads)])


def depth_encoder(depth, stack, residual=None):
    """stack(depth) [+ residual], (B, C, h, w) (see the module docstring)."""
    params = stack_parameters(stack)
    grad_on = torch.is_grad_enabled()
    if depth.requires_grad and grad_on:
        raise RuntimeError("depthg_amd: depth_encoder has no gradient for the depth map; detach it")
    if residual is not None and residual.requires_grad and grad_on:
        raise RuntimeError("depthg_amd: depth_encoder's `residual` is the frozen backbone's features and receives no gradient here; "
                           "detach it, or add it outside")
    ops.depth_encoder_shapes(depth, params, residual)
    if depth.is_cuda or any(p.is_cuda for p in params) or (residual is not None and residual.is_cuda):
        return _DepthEncoder.apply(depth, residual, *params)
    out = stack(depth.unsqueeze(1) if depth.dim() == 3 else depth)
    return out if residual is None else residual + out
