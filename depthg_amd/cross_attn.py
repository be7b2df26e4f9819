"""The depth guidance's cross-attention on fused HIP kernels (cfg.dg_fused_cross_attn; dg_xattn.hip).

cross_attention             dropout_p(softmax(q k^T * scale)) v per (batch, head), head dimension 48: on GPU tensors an autograd
                            function over ops.xattn_forward / ops.xattn_backward - the (B, heads, Nq, Nk) matrix is never stored,
                            the forward saves its output and the per-row log-sum-exp; on CPU tensors the plain torch formula.
multihead_cross_attention   the whole `cross_attn(query, kv, kv)[0]` of DepthGuidance._cross_attend on the parameters of an unchanged
                            nn.MultiheadAttention: the three input projections and out_proj are F.linear (ordinary GEMMs, torch's
                            autograd gives their parameter gradients), the fused core sits between them.

Random draws: the dropout mask is a Philox function of (seed, batch, head, query, key) - ops.xattn_keep_mask shows it - and NOT a
draw from torch's GPU generator, so with the flag on the head's Dropout2d draws no longer sit behind an attention-dropout draw in
that stream.  The seed itself comes from torch's CPU generator (ops._cpu_seed, as ops.super_perms): torch.manual_seed fixes it.
The seed is a kernel ARGUMENT: a captured graph replays the mask it was captured with.  A device-resident generator state that
would advance under replay is out of scope here.
"""
import math

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops

HEAD_DIM = ops.XATTN_HEAD_DIM


class _CrossAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads, p, scale, seed, want):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, lse = ops.xattn_forward(q, k, v, heads, p, seed, scale, want_lse=want)
        if want:
            ctx.save_for_backward(q, k, v, out, lse)
        ctx.conf = (heads, p, scale, seed)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors
        heads, p, scale, seed = ctx.conf
        gq, gk, gv = ops.xattn_backward(q, k, v, out, lse, grad_out.contiguous(), heads, p, seed, scale, need=ctx.needs_input_grad[:3])
        return gq, gk, gv, None, None, None, None, None


def _torch_cross_attention(q, k, v, heads, p, training, scale):
    B, Nq, C = q.shape
    hd = C // heads
    qh, kh, vh = (t.reshape(B, t.shape[1], heads, hd).transpose(1, 2) for t in (q, k, v))
    attn = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    attn = F.dropout(attn, p, training)
    return (attn @ vh).transpose(1, 2).reshape(B, Nq, C)


def cross_attention(q, k, v, heads, p=0.0, training=False, scale=None, seed=None):
    """q (B, Nq, heads * 48), k and v (B, Nk, heads * 48), batch-first -> (B, Nq, heads * 48).  p: the attention dropout, applied
    in training only; seed: None = drawn from torch's CPU generator when a mask is needed.  scale: None = 48 ** -0.5.  Under no_grad
    (or with no input that requires a gradient) the log-sum-exp is not written."""
    heads = int(heads)
    if q.dim() != 3 or heads < 1 or q.shape[2] != heads * HEAD_DIM:
        raise ValueError(f"depthg_amd: cross_attention: q must be (B, Nq, heads * {HEAD_DIM}) with heads={heads}, got {tuple(q.shape)}")
    p = float(p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f"depthg_amd: cross_attention: the dropout probability must be in [0, 1), got {p}")
    scale = HEAD_DIM ** -0.5 if scale is None else float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"depthg_amd: cross_attention: scale={scale}")
    if not q.is_cuda:
        return _torch_cross_attention(q, k, v, heads, p, training, scale)
    if p > 0.0 and seed is None:
        seed = ops._cpu_seed()
    want = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))       # a backward will follow: the forward writes the log-sum-exp
    return _CrossAttention.apply(q, k, v, heads, p, scale, 0 if seed is None else int(seed), want)


def check_module(mha):
    """ValueError unless `mha` is an nn.MultiheadAttention the fused core can stand in for."""
    why = None
    if not isinstance(mha, torch.nn.MultiheadAttention):
        why = f"a {type(mha).__name__}, not an nn.MultiheadAttention"
    elif mha.embed_dim % mha.num_heads or mha.embed_dim // mha.num_heads != HEAD_DIM:
        why = f"embed_dim / num_heads = {mha.embed_dim} / {mha.num_heads}, the kernels are built for head dimension {HEAD_DIM}"
    elif mha.batch_first:
        why = "batch_first=True (the guidance's module is sequence-first)"
    elif not mha._qkv_same_embed_dim or mha.in_proj_weight is None:
        why = f"kdim / vdim = {mha.kdim} / {mha.vdim} differ from embed_dim {mha.embed_dim}: there is no packed in_proj_weight"
    elif mha.in_proj_bias is None or mha.out_proj.bias is None:
        why = "built with bias=False"
    elif mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn:
        why = "add_bias_kv / add_zero_attn append keys the kernels do not know"
    if why:
        raise ValueError(f"depthg_amd: cfg.dg_fused_cross_attn cannot take this attention module: {why}")


def multihead_cross_attention(mha, query_map, image_feat, training, seed=None):
    """DepthGuidance._cross_attend: `mha(query, kv, kv)[0]` as a (B, C, h, w) map.  query_map: the queries as a (B, C, h, w) map, or
    one (C,) / (1, C) query for every position (the evaluation branch's no_depth_embed); image_feat (B, C, h, w): keys and values.
    p = mha.dropout, read here; the head-averaged attention weights nobody reads are not formed."""
    check_module(mha)
    B, C, fh, fw = image_feat.shape
    if C != mha.embed_dim:
        raise ValueError(f"depthg_amd: image_feat has {C} channels, the attention module embed_dim {mha.embed_dim}")
    kv = image_feat.reshape(B, C, fh * fw).transpose(1, 2)                     # (B, P, C) tokens, batch-first
    if query_map.dim() == 4:
        query = query_map.reshape(B, C, -1).transpose(1, 2)
    else:
        query = query_map.reshape(1, 1, C).expand(B, fh * fw, C)
    w, b = mha.in_proj_weight, mha.in_proj_bias
    q = F.linear(query, w[:C], b[:C])
    k = F.linear(kv, w[C:2 * C], b[C:2 * C])
    v = F.linear(kv, w[2 * C:], b[2 * C:])
    o = cross_attention(q, k, v, mha.num_heads, float(mha.dropout), training, None, seed)
    o = F.linear(o, mha.out_proj.weight, mha.out_proj.bias)
    return o.transpose(1, 2).reshape(B, C, fh, fw)
