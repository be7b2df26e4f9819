"""The DINO vision transformer the reference vendors (src/dino/vision_transformer.py:68-280), restated on torch: the frozen backbone
of DinoFeaturizer (src/modules.py:19-137).

Same contract as the reference's module:
    state_dict     the keys and shapes of a DINO checkpoint (cls_token, pos_embed, patch_embed.proj.*, blocks.{i}.norm1/attn.qkv/
                   attn.proj/norm2/mlp.fc1/mlp.fc2.*, norm.*), so `load_state_dict(strict=True)` takes one (:137-164)
    arithmetic     LayerNorm eps 1e-6, qkv bias, exact GELU, mlp ratio 4 (:262-280); position embeddings through the bicubic
                   interpolation with the +0.1 on the target size for every input other than the trained square (:179-199)
    methods        forward / forward_feats / get_intermediate_feat / get_last_selfattention / get_intermediate_layers (:214-259)
The dropout and drop-path layers of the reference are identities at their default rate 0, the only one DinoFeaturizer builds
(:30-32), and own no parameters: they are left out.

Attention has ONE entry point, `attention(qkv_packed, heads, scale, fused)`, on the packed output (B, N, 3 * heads * hd) of the qkv
linear.  fused = False is the reference's fp32 formulation in its order of operations (:82-89: the (B, heads, N, N) matrix is
materialised); fused = True (cfg.dg_fused_attention, off by default) is ops.attention_forward - the HIP kernel k_attn_fwd that
keeps the matrix on the compute unit (bf16 operands, fp32 softmax) and so returns no probabilities.  The callers decide: a block
asked for its attention probabilities is run with fused = False.

`fused_linear` (cfg.dg_fused_linear, off by default) runs the four linear layers of every block through ops.vit_linear_forward - the
HIP kernel k_lin_fwd (bf16 MFMA operands, fp32 accumulation) - as four launches: norm1 + qkv, proj + residual, norm2 + fc1 + GELU
(handed over as bf16), fc2 + residual.  The parameters stay the fp32 nn.Linear / nn.LayerNorm ones; the bf16 fragment-order copies
the kernel reads are a cache on the block (`Block._packs`), never part of state_dict(), rebuilt when a weight's storage or version
counter changes (load_state_dict, .to(device), an in-place edit).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


def attention(qkv_packed: torch.Tensor, heads: int, scale: float, fused: bool = False):
    """(B, N, 3 * heads * hd) -> (x (B, N, heads * hd), attn (B, heads, N, N), qkv (3, B, heads, N, hd) view).
    src/dino/vision_transformer.py:82-89.  fused: the HIP kernel instead; attn is then None."""
    B, N, C3 = qkv_packed.shape
    hd = C3 // (3 * heads)
    qkv = qkv_packed.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    if fused:
        return ops.attention_forward(qkv_packed, heads, scale), None, qkv
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = (q @ k.transpose(-2, -1)) * scale
    attn = attn.softmax(dim=-1)
    x = (attn @ v).transpose(1, 2).reshape(B, N, heads * hd)
    return x, attn, qkv


class Mlp(nn.Module):
    """fc1 -> exact GELU -> fc2 (:49-65)."""

    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Attention(nn.Module):
    """:68-92.  forward returns (x, attn, qkv); attn is None when the fused kernel ran."""

    def __init__(self, dim, num_heads, qkv_bias=True, qk_scale=None):
        super().__init__()
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, fused=False):
        x, attn, qkv = attention(self.qkv(x), self.num_heads, self.scale, fused)
        return self.proj(x), attn, qkv


class Block(nn.Module):
    """:95-115."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=True, qk_scale=None, eps=1e-6):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, num_heads, qkv_bias, qk_scale)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def packed_weight(self, name):
        """The bf16 fragment-order copy of the weight of qkv / proj / fc1 / fc2 (ops.vit_linear_pack), packed at first use and again
        whenever the parameter's storage or version counter is not the one it was packed from."""
        w = self._linear(name).weight
        key = (w.data_ptr(), w._version, w.device)
        hit = self.__dict__.setdefault("_packs", {}).get(name)
        if hit is None or hit[0] != key:
            hit = (key, ops.vit_linear_pack(w.detach()))
            self._packs[name] = hit
        return hit[1]

    def _apply(self, fn, *args, **kwargs):
        """.to(device) / .cpu() / .float(): the parameters move, the packs of the old ones are dropped (the allocator may hand the
        new storage the old address)."""
        self.__dict__.pop("_packs", None)
        return super()._apply(fn, *args, **kwargs)

    def pack_is_stale(self, name):
        """True when the next fused forward will pack the weight of `name` (again)."""
        w, hit = self._linear(name).weight, self.__dict__.get("_packs", {}).get(name)
        return hit is None or hit[0] != (w.data_ptr(), w._version, w.device)

    def _linear(self, name):
        return {"qkv": self.attn.qkv, "proj": self.attn.proj, "fc1": self.mlp.fc1, "fc2": self.mlp.fc2}[name]

    def _fused_linear(self, name, x, norm=None, **kw):
        lin = self._linear(name)
        if norm is not None:
            kw.update(ln_weight=norm.weight, ln_bias=norm.bias, eps=norm.eps)
        return ops.vit_linear_forward(x, self.packed_weight(name), lin.out_features, lin.bias, **kw)

    def _forward_fused_linear(self, x, return_attention, return_qkv, fused):
        """The block as four launches of k_lin_fwd around the attention.  `x` is left as it is: proj writes a fresh residual
        stream, fc2 adds into that one in place."""
        x = x.contiguous()
        qkv_packed = self._fused_linear("qkv", x, self.norm1)
        y, attn, qkv = attention(qkv_packed, self.attn.num_heads, self.attn.scale, fused and not return_attention)
        if return_attention:
            return attn
        x = self._fused_linear("proj", y.contiguous(), residual=x)
        hidden = self._fused_linear("fc1", x, self.norm2, gelu=True, out_bf16=True)
        x = self._fused_linear("fc2", hidden, residual=x, out=x)
        return (x, attn, qkv) if return_qkv else x

    def forward(self, x, return_attention=False, return_qkv=False, fused=False, fused_linear=False):
        """fused: this block's attention through the HIP kernel.  It yields no probabilities, so return_attention overrides it
        and a fused return_qkv hands back (x, None, qkv).  fused_linear: the linear layers through the HIP kernel."""
        if fused_linear:
            return self._forward_fused_linear(x, return_attention, return_qkv, fused)
        y, attn, qkv = self.attn(self.norm1(x), fused=fused and not return_attention)
        if return_attention:
            return attn
        x = x + y
        x = x + self.mlp(self.norm2(x))
        return (x, attn, qkv) if return_qkv else x


class PatchEmbed(nn.Module):
    """:118-134."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.img_size, self.patch_size = img_size, patch_size
        self.num_patches = (img_size // patch_size) * (img_size // patch_size)
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class VisionTransformer(nn.Module):
    """:137-259.  `fused_attention`: the blocks' attention through ops.attention_forward (GPU only; head dimension 64).
    `fused_linear`: the blocks' linear layers through ops.vit_linear_forward (GPU only; widths that are multiples of 64)."""

    def __init__(self, img_size=(224,), patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, eps=1e-6, fused_attention=False, fused_linear=False):
        super().__init__()
        self.num_features = self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.fused_attention = bool(fused_attention)
        if self.fused_attention and embed_dim // num_heads != 64:
            raise ValueError(f"depthg_amd: the fused attention kernel is built for head dimension 64, got {embed_dim // num_heads}")
        self.fused_linear = bool(fused_linear)
        if self.fused_linear:
            hidden = int(embed_dim * mlp_ratio)
            for what, k, n in (("embed_dim", embed_dim, 3 * embed_dim), ("mlp hidden width", hidden, embed_dim)):
                if not ops.vit_linear_supported(k, n):
                    raise ValueError(f"depthg_amd: the fused linear kernel is built for layer widths that are multiples of 64 up to "
                                     f"{ops.VIT_LINEAR_MAX}, got {what} = {k} (a {k} -> {n} layer)")
            if embed_dim > 768:
                raise ValueError(f"depthg_amd: the fused linear kernel's LayerNorm prologue is built for embed_dim <= 768, got {embed_dim}")
        self.patch_embed = PatchEmbed(img_size[0], patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias, qk_scale, eps) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=eps)
        nn.init.trunc_normal_(self.pos_embed, std=.02)                     # :166-177
        nn.init.trunc_normal_(self.cls_token, std=.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def interpolate_pos_encoding(self, x, w, h):
        """:179-199 (w, h are the image's dims 2 and 3, as the reference names them)."""
        npatch, n = x.shape[1] - 1, self.pos_embed.shape[1] - 1
        if npatch == n and w == h:
            return self.pos_embed
        side, dim = int(math.sqrt(n)), x.shape[-1]
        w0, h0 = w // self.patch_embed.patch_size + 0.1, h // self.patch_embed.patch_size + 0.1
        grid = self.pos_embed[:, 1:].reshape(1, side, side, dim).permute(0, 3, 1, 2)
        grid = F.interpolate(grid, scale_factor=(w0 / math.sqrt(n), h0 / math.sqrt(n)), mode="bicubic")
        assert int(w0) == grid.shape[-2] and int(h0) == grid.shape[-1]
        return torch.cat((self.pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, -1, dim)), dim=1)

    def prepare_tokens(self, x):
        """:201-212."""
        B, _, w, h = x.shape
        x = self.patch_embed(x)
        x = torch.cat((self.cls_token.expand(B, -1, -1), x), dim=1)
        return x + self.interpolate_pos_encoding(x, w, h)

    def forward_feats(self, x):
        """All tokens after the final norm (:221-226)."""
        x = self.prepare_tokens(x)
        for blk in self.blocks:
            x = blk(x, fused=self.fused_attention, fused_linear=self.fused_linear)
        return self.norm(x)

    def forward(self, x):
        """The class token (:214-219)."""
        return self.forward_feats(x)[:, 0]

    def get_intermediate_feat(self, x, n=1, want_attn=True):
        """(feat, attns, qkvs) of the last n blocks (:228-240); qkv is (3, B, heads, N, hd).  want_attn = False (not in the
        reference): nobody will read the probabilities, so the recorded blocks may run fused too and their `attns` entry is None."""
        x = self.prepare_tokens(x)
        feat, attns, qkvs = [], [], []
        for i, blk in enumerate(self.blocks):
            if len(self.blocks) - i <= n:
                x, attn, qkv = blk(x, return_qkv=True, fused=self.fused_attention and not want_attn, fused_linear=self.fused_linear)
                feat.append(self.norm(x)); attns.append(attn); qkvs.append(qkv)
            else:
                x = blk(x, fused=self.fused_attention, fused_linear=self.fused_linear)
        return feat, attns, qkvs

    def get_last_selfattention(self, x):
        """:242-249."""
        x = self.prepare_tokens(x)
        for blk in self.blocks[:-1]:
            x = blk(x, fused=self.fused_attention, fused_linear=self.fused_linear)
        return self.blocks[-1](x, return_attention=True, fused_linear=self.fused_linear)

    def get_intermediate_layers(self, x, n=1):
        """:251-259."""
        x = self.prepare_tokens(x)
        out = []
        for i, blk in enumerate(self.blocks):
            x = blk(x, fused=self.fused_attention, fused_linear=self.fused_linear)
            if len(self.blocks) - i <= n:
                out.append(self.norm(x))
        return out


def vit_tiny(patch_size=16, **kw):
    """:262-266."""
    return VisionTransformer(patch_size=patch_size, **{**dict(embed_dim=192, depth=12, num_heads=3), **kw})


def vit_small(patch_size=16, **kw):
    """:269-273."""
    return VisionTransformer(patch_size=patch_size, **{**dict(embed_dim=384, depth=12, num_heads=6), **kw})


def vit_base(patch_size=16, **kw):
    """:276-280."""
    return VisionTransformer(patch_size=patch_size, **{**dict(embed_dim=768, depth=12, num_heads=12), **kw})


ARCHS = {"vit_tiny": vit_tiny, "vit_small": vit_small, "vit_base": vit_base}

# the checkpoints the reference fetches when none is given (src/modules.py:41-48) - named in the warning, never opened here
CHECKPOINT_NAMES = {("vit_small", 16): "dino_deitsmall16_pretrain.pth", ("vit_small", 8): "dino_deitsmall8_300ep_pretrain.pth",
                    ("vit_base", 16): "dino_vitbase16_pretrain.pth", ("vit_base", 8): "dino_vitbase8_pretrain.pth"}


def load_checkpoint(model: nn.Module, path: str):
    """src/modules.py:52-64: a local file holding {"teacher": state} (prefixes `module.` and `backbone.` removed, strict=False) -
    or a plain state dict, taken the same way.  Returns load_state_dict's message."""
    state = torch.load(path, map_location="cpu")
    if isinstance(state, dict) and "teacher" in state:
        state = state["teacher"]
    state = {k.replace("module.", "").replace("backbone.", ""): v for k, v in state.items()}
    return model.load_state_dict(state, strict=False)
