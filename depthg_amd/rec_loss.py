"""The reconstruction loss term of the training step (src/train_segmentation.py:391-398 under cfg.rec_weight): STEGO's auxiliary
decoder - a 1 x 1 convolution from the code back to the backbone's features (src/train_segmentation.py:115) - must point along the
features it came from.

    reconstruction_loss(code, feats, weight, bias)     the scalar
        rec_feats = conv2d(code, weight, bias)                                   :392 (self.decoder(code))
        loss      = -(norm(rec_feats) * norm(feats)).sum(1).mean()               :393; src/modules.py:789-790 (F.normalize(dim=1, eps=1e-10))
      code (B,D,h,w) = net(img)[1], feats (B,C,h,w) = net(img)[0] - a tensor or an ops.DeferredDropout, whose Dropout2d is then
      applied inside the kernels - weight (C,D,1,1) or (C,D) and bias (C,) the decoder's.  On GPU tensors: one fused HIP forward and
      one HIP backward (ops.rec_loss_forward / rec_loss_backward, dg_rec_loss.hip) tied together by a torch.autograd.Function;
      gradients go to code, weight and bias, and no (B,C,h,w) tensor is written in either direction.  feats is the frozen backbone's
      output and receives none.  On CPU tensors: the plain differentiable torch chain above, any floating dtype.

    reconstruction_loss(code, feats, weight, bias, feats_grad=True)
      the same scalar, and feats - or the maps of an ops.DeferredDropout - may require grad and then receive d loss / d feats
      = a y + b' f (include/depthg_corr.h), written by the kernel that forms d code from the registers it holds (one more (B,C,h,w)
      store, ops.rec_loss_backward(want_feats=True), dg_rec_feats_backward): DinoFeaturizerWithDepth's feats are attached to its
      trained depth modules (src/modules.py:596-598), which the term trains through them.  Gradients are returned per
      needs_input_grad; without a feats that asks, the route and the bits are those of the call without the keyword.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops


class _Reconstruction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, code, weight, bias, feats, keep, scale):
        # contiguous float32 once: the kernels of both directions read these, and a strided input is copied here and nowhere else
        c, f, w, b, k, scale, _ = ops._rec_loss_operands(code, feats, weight, bias, keep, scale)
        loss, ws = ops.rec_loss_forward(c, f, w, b, k, scale)
        ctx.ws, ctx.scale, ctx.weight_shape, ctx.feats_shape = ws, scale, weight.shape, feats.shape
        ctx.save_for_backward(c, w, b, f, k)
        return loss

    @staticmethod
    @once_differentiable              # (the kernels give the three first derivatives and nothing of higher order)
    def backward(ctx, grad_out):
        code, weight, bias, feats, keep = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_feats = None
        if need[3]:                       # (reconstruction_loss lets a feats that requires grad through under feats_grad=True alone)
            d_code, d_weight, d_bias, d_feats = ops.rec_loss_backward(ctx.ws, code, feats, weight, bias, grad_out, keep, ctx.scale,
                                                                      want_feats=True, want_params=any(need[:3]))
            d_feats = d_feats.view(ctx.feats_shape)
        else:
            d_code, d_weight, d_bias = ops.rec_loss_backward(ctx.ws, code, feats, weight, bias, grad_out, keep, ctx.scale)
        return (d_code if need[0] else None), (d_weight.view(ctx.weight_shape) if need[1] else None), (d_bias if need[2] else None), \
            d_feats, None, None


def reconstruction_loss(code, feats, weight, bias, feats_grad=False):
    """-mean <norm(conv2d(code, weight, bias)), norm(feats)>, a 0-dim tensor (see the module docstring).  feats_grad: a feats
    (or DeferredDropout maps) that requires grad is accepted and receives its gradient; False refuses it."""
    deferred = isinstance(feats, ops.DeferredDropout)
    maps = feats.feats if deferred else feats
    if maps.requires_grad and torch.is_grad_enabled() and not feats_grad:
        raise RuntimeError("depthg_amd: reconstruction_loss has no gradient for `feats` (the frozen backbone's output); detach it")
    weight2d, (_, D, C, _, _) = ops.rec_loss_shapes(code, maps, weight, bias)
    tensors = ((code, "code"), (maps, "feats"), (weight, "weight"), (bias, "bias"))
    if any(t.is_cuda for t, _ in tensors):
        ops._gpu_float32(tensors, "reconstruction_loss wants float32 tensors on the GPU, got {name} as {dtype}")
        keep, scale = (feats.keep, feats.scale) if deferred else (None, 1.0)
        return _Reconstruction.apply(code, weight, bias, maps, keep, scale)      # (D > 128 is refused there, before any launch)
    if deferred:                          # (materialize() is differentiable: the maps of a DeferredDropout get theirs through it)
        maps = feats.materialize().to(maps.dtype)
    rec_feats = F.conv2d(code, weight2d.reshape(C, D, 1, 1), bias)
    return -(F.normalize(rec_feats, dim=1, eps=1e-10) * F.normalize(maps, dim=1, eps=1e-10)).sum(1).mean()
