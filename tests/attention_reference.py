"""Restatement for the tests of the fused attention kernel (depthg_amd/csrc/dg_attn.hip, ops.attention_forward) and of
cfg.dg_fused_attention.  Not imported by the product.

    truth       softmax(q k^T * scale) v (src/dino/vision_transformer.py:80-92) in float64 torch
    yardstick   the same float64 computation on q, k, v rounded to bf16: the error no kernel with bf16 operands can avoid
    criterion   relative L2 error of the kernel against truth <= 1.5 x the yardstick's.  The factor: an emulation of the prescribed
                arithmetic (bf16 operands, fp32 scores and softmax, P rounded to bf16, fp32 accumulation) lands at 1.01-1.17 x the
                yardstick for N in {65, 785, 1601}, sigma in {1, 3}; 1.5 x leaves room for the accumulation order and nothing else.
    model       a vit.VisionTransformer whose attention rounds q, k, v to bf16 inside the fp32 torch formulation: the yardstick
                of the whole-model comparison.
"""
import torch

FACTOR = 1.5


def split_qkv(qkv_packed, heads):
    """(B, N, 3 * heads * hd) -> q, k, v (B, heads, N, hd), as :82-83."""
    B, N, C3 = qkv_packed.shape
    qkv = qkv_packed.reshape(B, N, 3, heads, C3 // (3 * heads)).permute(2, 0, 3, 1, 4)
    return qkv[0], qkv[1], qkv[2]


def attention_f64(qkv_packed, heads, scale, round_bf16=False):
    """Truth (round_bf16 = False) or yardstick (True): float64 on the tensor's device, chunked over (batch, head) so that the
    N x N matrix of one head is all that lives at once.  Returns (B, N, heads * hd) float64."""
    q, k, v = split_qkv(qkv_packed, heads)
    B, H, N, hd = q.shape
    out = torch.empty(B, N, H * hd, dtype=torch.float64, device=qkv_packed.device)
    for b in range(B):
        for h in range(H):
            qq, kk, vv = (t[b, h].to(torch.bfloat16).double() if round_bf16 else t[b, h].double() for t in (q, k, v))
            out[b, :, h * hd:(h + 1) * hd] = torch.softmax(qq @ kk.t() * scale, dim=-1) @ vv
    return out


def rel_l2(got, truth):
    return float((got.double() - truth).norm() / truth.norm())


def ratios(got, qkv_packed, heads, scale):
    """(kernel error, yardstick error) against the float64 truth, both relative L2."""
    truth = attention_f64(qkv_packed, heads, scale)
    return rel_l2(got, truth), rel_l2(attention_f64(qkv_packed, heads, scale, True), truth)


def seeded_qkv(B, N, heads, sigma, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (sigma * torch.randn(B, N, 3 * heads * 64, generator=g)).to(device)


def dominant_qkv(B, N, heads, j, seed, device="cpu"):
    """Every query is 40 x key j: one score dominates each row (40 |k_j|^2 / 8, about 320), the expected output is v_j.  A softmax
    without the running maximum overflows on it."""
    qkv = seeded_qkv(B, N, heads, 1.0, seed).reshape(B, N, 3, heads, 64)
    qkv[:, :, 0] = 40.0 * qkv[:, j:j + 1, 1]
    return qkv.reshape(B, N, 3 * heads * 64).contiguous().to(device)


def bf16_operand_model(model):
    """The whole-model yardstick: `model` (a vit.VisionTransformer, left untouched) copied with an attention that rounds q, k, v to
    bf16 and then runs the fp32 torch formulation."""
    import copy
    from depthg_amd import vit
    m = copy.deepcopy(model)
    m.fused_attention = False

    def rounded(self, x, fused=False):
        p = self.qkv(x)
        y, attn, qkv = vit.attention(p.to(torch.bfloat16).to(torch.float32), self.num_heads, self.scale)
        return self.proj(y), attn, qkv

    for blk in m.blocks:
        blk.attn.forward = rounded.__get__(blk.attn)
    return m


# ---- seeded weights of the ViT fixtures (tests/golden/make_vit_fixtures.py draws them, the tests re-draw them: vit.npz stores the
# seed and a checksum, not the 1.7 MB state dict)
TINY = dict(img_size=[32], patch_size=8, embed_dim=128, depth=2, num_heads=2)          # head dimension 64
TINY6 = dict(img_size=[32], patch_size=8, embed_dim=384, depth=1, num_heads=6)         # six heads: what "KK" hard-codes (src/modules.py:113)


def seeded_tensors(named_shapes, seed):
    """{name: tensor} in the given order from one generator: LayerNorm / norm weights 1 + 0.1 randn, everything else 0.05 randn."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in named_shapes:
        t = torch.randn(tuple(shape), generator=g)
        is_norm_weight = name.endswith("weight") and name.split(".")[-2] in ("norm", "norm1", "norm2")
        out[name] = 1.0 + 0.1 * t if is_norm_weight else 0.05 * t
    return out


def checksum(tensors):
    ts = list(tensors.values())
    return [float(sum(t.double().sum() for t in ts)), float(sum(t.double().abs().sum() for t in ts))]


def seed_module(module, seed, expect=None):
    """Load seeded_tensors into `module` (strict); with `expect` the stored checksum must match the draw."""
    import numpy as np
    state = seeded_tensors([(k, v.shape) for k, v in module.state_dict().items()], seed)
    if expect is not None:
        assert np.allclose(checksum(state), expect, rtol=1e-12, atol=1e-9), "the seeded weights differ from the ones the reference ran on"
    module.load_state_dict(state, strict=True)
    return module
