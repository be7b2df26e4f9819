"""DinoFeaturizer (src/modules.py:19-137): the frozen DINO ViT of depthg_amd/vit.py, the reference's feature selection and the
projection head as one fused HIP launch (depthg_amd/head.py run_head / run_head_pair).

Differences from the reference, all on the build side:
    weights     cfg.pretrained_weights names a LOCAL file (the reference's `{"teacher": ...}` checkpoint, :52-64, or a plain state
                dict).  With None the reference downloads (:65-68); this module never opens a network connection: the ViT keeps its
                random initialisation and a warning names the checkpoint to supply.
    attention   the (B, heads, N, N) probabilities of the last block are returned in training mode only when something reads them
                (cfg.lhp with propagation_strategy == "attn", src/train_segmentation.py:202-203); otherwise the one-element
                placeholder StandInFeaturizer returns.  cfg.dg_fused_attention (off by default) routes every block whose
                probabilities nobody reads through the fused HIP kernel (ops.attention_forward).
    linears     cfg.dg_fused_linear (off by default) runs the four linear layers of every block, with the LayerNorm, GELU and
                residual add around them, through the bf16 MFMA kernel (ops.vit_linear_forward); the weights stay fp32 parameters.
    "KK"        the reference hard-codes 6 heads (:113); the head count of the model is used (the same for ViT-S).
    backbone    cfg.dg_dino_vit_kwargs (None, or a dict) overrides the architecture's constructor arguments: the test hook that builds
                small backbones.

DinoFeaturizerWithDepth (src/modules.py:490-631, cfg.arch "dino_depth"): the same frozen backbone with a trainable depth encoder
(`depth_downscaling`) whose feature-resolution map is mixed into the DINO features in front of the head - cfg.guidance "sum",
"cross_attn" (`cross_attn`, `no_depth_embed`), "concat" or "none".  The head runs as ever (run_head) with input_grad=True: its
d image_feat launch (dg_head_backward_input) carries the gradient into the depth modules, which are plain torch - except, with
cfg.dg_fused_depth_encoder (off by default; n_feats == 384 only), the depth encoder: one fused HIP forward and backward
(depth_encoder.py, dg_depth_enc.hip), the "sum" guidance's add in its epilogue - and, with cfg.dg_fused_cross_attn (off by
default; n_feats == 384 only), the core of the "cross_attn" guidance's attention (cross_attn.py, dg_xattn.hip): `cross_attn` stays
the reference's nn.MultiheadAttention (same parameters, state dict and initial values), its projections run as F.linear, and the
softmax(q k^T) v between them, with its dropout, is one fused HIP forward and backward.  With that flag on, the attention dropout's
mask is a Philox function of a seed drawn from torch's CPU generator, not a draw from torch's GPU stream: the head's Dropout2d draws
no longer sit behind it.  The seed is a kernel argument, so a captured graph replays the mask it was captured with; a
device-resident generator state for it is out of scope.  DepthGuidance is the
guidance logic as a mixin over any FrozenBackboneFeaturizer (segmenter.StandInFeaturizerWithDepth is the stand-in variant).
Differences from the reference:
    concat      the reference's training branch is `pass` (:564-565) and leaves image_depth_feat unbound; here "concat" is "none".
    unused work depth_downscaling is not run where its result is unused (:557 runs it always): "none", "concat", and eval mode, where
                the reference feeds it zeros (:613) that "sum" / "none" then ignore.
    frozen      parameters the chosen guidance never touches in training are built (the state dict is the reference's) but have
                requires_grad = False: an optimiser never meets a parameter without a gradient - what torch's Adam does with
                `grad is None` in the reference, skipping it.
    image_feat  the third training-mode return value is the (B, C, h, w) map under every guidance (under "cross_attn" the reference
                returns its sequence-first view, :568; nothing reads it).
"""
import warnings

import torch
import torch.nn as nn

from . import vit
from .cross_attn import check_module, multihead_cross_attention
from .depth_encoder import depth_encoder
from .head import ProjectionHead, run_head, run_head_pair


class FrozenBackboneFeaturizer(nn.Module):
    """DinoFeaturizer's output contract (src/modules.py:90-137: train -> (feats, code, attn), eval -> (feats, code); feats get a
    third Dropout2d mask when cfg.dropout) around any frozen backbone.  A subclass sets `cfg`, `patch_size`, `n_feats` and `model`,
    calls `_register_head`, and supplies `_backbone(img, n, return_class_feat)` -> (image_feat (B, n_feats, H/p, W/p), attn), or
    (the class feature (B, n_feats, 1, 1), None); it runs under no_grad with the backbone in eval mode."""

    supports_deferred_dropout = True      # forward_pair(..., defer_feats_dropout=True) hands back ops.DeferredDropout feats

    def _register_head(self, dim, cfg):
        """Dropout2d, cluster1 and cluster2 under the reference's names (:75-88), behind `model`: its checkpoints load unchanged."""
        self.dropout = nn.Dropout2d(p=.1)
        head = ProjectionHead(self.n_feats, dim, getattr(cfg, "projection_type", "nonlinear"))   # (modules only: run_head does the work)
        self.cluster1 = head.cluster1
        if hasattr(head, "cluster2"):
            self.cluster2 = head.cluster2
        self.proj_type = head.proj_type

    def _head_modules(self):
        return self.cluster1, self.cluster2 if self.proj_type == "nonlinear" else None

    def forward(self, img, n=1, return_class_feat=False):
        self.model.eval()
        with torch.no_grad():
            image_feat, attn = self._backbone(img, n, return_class_feat)
            if return_class_feat:
                return image_feat
        return self.forward_features(image_feat, attn)

    def forward_features(self, image_feat, attn=None):
        """forward() behind the backbone (:122-137), from its `image_feat` (B, n_feats, h, w) - the backbone's own, or the rows a
        feature_cache.FeatureCache kept of it (`attn` is then None: no attention map was stored)."""
        if self.proj_type is not None:
            # one fused HIP launch: code = cluster1(drop(f)) [+ cluster2(drop(f))] and feats = drop(f) (:122-137; three draws)
            code, feats = run_head(*self._head_modules(), image_feat, self.training, bool(self.cfg.dropout), float(self.dropout.p))
        else:
            code = image_feat
            feats = self.dropout(image_feat) if self.cfg.dropout else image_feat    # :129-137 (identity in eval mode)
        return (feats, code, attn) if self.training else (feats, code)

    def forward_pair(self, img, img_pos, defer_feats_dropout=False):
        """forward(img) and forward(img_pos) of one training step (src/train_segmentation.py:194-212) with the head's two passes in
        one set of launches (run_head_pair): the frozen backbone has no random draws, so the six Dropout2d draws come in the
        reference's order.  Training mode with a projection head only; returns ((feats, code, attn), (feats_pos, code_pos, attn_pos))."""
        if not self.training or self.proj_type is None:
            return self.forward(img), self.forward(img_pos)
        self.model.eval()
        with torch.no_grad():
            (image_feat, attn), (image_feat_pos, attn_pos) = self._backbone(img), self._backbone(img_pos)
        return self.forward_pair_features(image_feat, image_feat_pos, defer_feats_dropout, attn, attn_pos)

    def forward_pair_features(self, image_feat, image_feat_pos, defer_feats_dropout=False, attn=None, attn_pos=None):
        """forward_pair() behind the backbone, from the two passes' `image_feat` - the backbone's own, or a FeatureCache's rows (the
        attention maps are then None).  The Dropout2d draws come as forward_pair's do."""
        if not self.training or self.proj_type is None:
            return self.forward_features(image_feat, attn), self.forward_features(image_feat_pos, attn_pos)
        (code, feats), (code_pos, feats_pos) = run_head_pair(*self._head_modules(), image_feat, image_feat_pos, True,
                                                             bool(self.cfg.dropout), float(self.dropout.p), None, defer_feats_dropout)
        return (feats, code, attn), (feats_pos, code_pos, attn_pos)


class LayerNorm2d(nn.Module):
    """src/modules.py:619-631: normalisation over the channels of a (B, C, H, W) map, biased variance, eps inside the root."""

    def __init__(self, num_channels: int, eps: float = 1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))
        self.eps = eps

    def forward(self, x):
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        x = (x - u) / torch.sqrt(s + self.eps)
        return self.weight[:, None, None] * x + self.bias[:, None, None]


GUIDANCES = ("cross_attn", "concat", "sum", "none")                             # src/modules.py:528


def make_depth_downscaling(n_feats: int) -> nn.Sequential:
    """src/modules.py:497-522: 2 x 2 stride-2 convolutions with LayerNorm2d + GELU between them - three stages (a factor 8, the
    patch size) for n_feats == 384, five (a factor 32) otherwise."""
    widths = (1, 64, 128, n_feats) if n_feats == 384 else (1, 64, 128, 256, 512, n_feats)
    layers = []
    for i, (cin, cout) in enumerate(zip(widths[:-1], widths[1:])):
        layers.append(nn.Conv2d(cin, cout, kernel_size=2, stride=2))
        if i < len(widths) - 2:
            layers += [LayerNorm2d(cout), nn.GELU()]
    return nn.Sequential(*layers)


class DepthGuidance:
    """DinoFeaturizerWithDepth's depth modules and forward (src/modules.py:495-614) over a FrozenBackboneFeaturizer: list it in
    front of the featurizer class and call `_register_depth(cfg)` behind the featurizer's own __init__ (the head's initial values
    then equal the plain featurizer's under the same seed).  Training input (img, depth) -> (feats, code, image_feat, attn); eval
    input img -> (feats, code, attn).  forward_pair and deferred dropout are not offered."""

    supports_deferred_dropout = False

    def _register_depth(self, cfg):
        self.guidance = getattr(cfg, "guidance", "none")                        # :526
        if self.guidance not in GUIDANCES:                                      # :528
            raise ValueError(f"depthg_amd: cfg.guidance must be one of {GUIDANCES}, got {self.guidance!r}")
        self.depth_downscaling = make_depth_downscaling(self.n_feats)           # :497-522
        self.cross_attn = nn.MultiheadAttention(embed_dim=self.n_feats, num_heads=8, dropout=0.1)    # :524 (sequence-first)
        self.no_depth_embed = nn.Embedding(1, self.n_feats)                     # :530
        self.fused_depth_encoder = bool(getattr(cfg, "dg_fused_depth_encoder", False))
        if self.fused_depth_encoder and self.n_feats != 384:
            raise ValueError(f"depthg_amd: cfg.dg_fused_depth_encoder fuses the three-stage depth encoder of n_feats == 384; this backbone "
                             f"has n_feats = {self.n_feats}, whose five-stage stack stays on the torch route: leave the flag off")
        self.fused_cross_attn = bool(getattr(cfg, "dg_fused_cross_attn", False))
        if self.fused_cross_attn:
            if self.n_feats != 384:
                raise ValueError(f"depthg_amd: cfg.dg_fused_cross_attn fuses the 8-heads-of-48 attention of n_feats == 384; this backbone has "
                                 f"n_feats = {self.n_feats} (head dimension {self.n_feats / 8:g}), which stays on the torch route: leave the flag off")
            check_module(self.cross_attn)
        frozen = {"none": (self.depth_downscaling, self.cross_attn, self.no_depth_embed),
                  "concat": (self.depth_downscaling, self.cross_attn, self.no_depth_embed),
                  "sum": (self.cross_attn, self.no_depth_embed),
                  "cross_attn": (self.no_depth_embed,)}[self.guidance]
        for m in frozen:
            for p in m.parameters():
                p.requires_grad = False

    def depth_parameters(self):
        """{name: parameter} of the depth modules (trainable or not)."""
        return {n: p for n, p in self.named_parameters() if n.split(".")[0] in ("depth_downscaling", "cross_attn", "no_depth_embed")}

    def _depth_feats(self, depth, image_feat, residual=None):
        """depth_downscaling(depth) (+ residual); with cfg.dg_fused_depth_encoder one fused HIP forward (depth_encoder.py)."""
        if depth.dim() == 3:
            depth = depth.unsqueeze(1)
        if self.fused_depth_encoder:
            if tuple(depth.shape[2:]) != (8 * image_feat.shape[2], 8 * image_feat.shape[3]):
                raise ValueError(f"depthg_amd: the depth map {tuple(depth.shape)} is not 8 x the backbone's feature grid {tuple(image_feat.shape)}: "
                                 f"the depth must come at the image's resolution and the patch size ({self.patch_size}) must be 8")
            return depth_encoder(depth.to(image_feat.dtype), self.depth_downscaling, residual)
        depth_feats = self.depth_downscaling(depth.to(image_feat.dtype))        # :557
        if depth_feats.shape != image_feat.shape:
            raise ValueError(f"depthg_amd: depth_downscaling turns the depth map {tuple(depth.shape)} into {tuple(depth_feats.shape)}, "
                             f"the backbone's features are {tuple(image_feat.shape)}: the depth must come at the image's resolution "
                             f"and the stack must shrink it by the patch size ({self.patch_size})")
        return depth_feats if residual is None else residual + depth_feats

    def _cross_attend(self, query, image_feat):
        """:568-575 / :577-585: cross_attn(query, image_feat, image_feat) on sequence-first tokens, back as a (B, C, h, w) map."""
        B, C, fh, fw = image_feat.shape
        kv = image_feat.reshape(B, C, -1).permute(2, 0, 1)
        return self.cross_attn(query, kv, kv)[0].permute(1, 2, 0).reshape(B, C, fh, fw)

    def forward(self, input, n=1, return_class_feat=False, keeps=None):
        """`keeps`: the head's three Dropout2d keep masks (head.draw_keep_masks) instead of fresh draws - the test hook run_head has."""
        if self.training:                                                       # :607-614
            if not isinstance(input, (tuple, list)) or len(input) != 2:
                raise ValueError("Input should be a tuple of (image, depth)")
            img, depth = input
        else:
            img, depth = (input[0] if isinstance(input, (tuple, list)) else input), None
        self.model.eval()
        with torch.no_grad():
            image_feat, attn = self._backbone(img, n, return_class_feat)
            if return_class_feat:
                return image_feat
        B, C = image_feat.shape[:2]
        if self.training and self.guidance == "sum":                            # :562-563
            image_depth_feat = self._depth_feats(depth, image_feat, image_feat)    # (fused: the add runs in the kernel's epilogue)
        elif self.training and self.guidance == "cross_attn" and self.fused_cross_attn:
            image_depth_feat = multihead_cross_attention(self.cross_attn, self._depth_feats(depth, image_feat), image_feat, True)
        elif self.guidance == "cross_attn" and self.fused_cross_attn:
            image_depth_feat = multihead_cross_attention(self.cross_attn, self.no_depth_embed.weight, image_feat, False)
        elif self.training and self.guidance == "cross_attn":                   # :566-575
            image_depth_feat = self._cross_attend(self._depth_feats(depth, image_feat).reshape(B, C, -1).permute(2, 0, 1), image_feat)
        elif self.guidance == "cross_attn":                                     # :576-585: no depth at evaluation, a learned query
            P = image_feat.shape[2] * image_feat.shape[3]
            image_depth_feat = self._cross_attend(self.no_depth_embed.weight.reshape(1, 1, -1).expand(P, B, -1), image_feat)
        else:                                                                   # :586-587
            image_depth_feat = image_feat
        if self.proj_type is not None:
            # :589-605 - the fused head; its three Dropout2d draws come behind whatever cross_attn's own dropout drew, as there
            # (cfg.dg_rec_feats_grad: the returned feats stay attached, for the reconstruction term to train the depth modules through)
            code, feats = run_head(*self._head_modules(), image_depth_feat, self.training, bool(self.cfg.dropout), float(self.dropout.p),
                                   keeps, input_grad=True, feats_grad=bool(getattr(self.cfg, "dg_rec_feats_grad", False)))
        else:
            code = image_depth_feat
            feats = self.dropout(image_depth_feat) if self.cfg.dropout else image_depth_feat
        return (feats, code, image_feat, attn) if self.training else (feats, code, attn)

    def forward_pair(self, *args, **kwargs):
        raise NotImplementedError("depthg_amd: the depth-guided featurizer has no paired pass (call it once per image set)")

    def forward_features(self, *args, **kwargs):
        raise NotImplementedError("depthg_amd: the depth-guided featurizer mixes the depth map in behind the backbone: it has no pass "
                                  "from cached features (cfg.dg_feature_cache serves cfg.arch = 'dino')")

    forward_pair_features = forward_features


class DinoFeaturizer(FrozenBackboneFeaturizer):
    """DinoFeaturizer(dim, cfg) of src/modules.py:19-137."""

    def __init__(self, dim: int, cfg):
        super().__init__()
        self.cfg, self.dim = cfg, dim
        self.patch_size = int(cfg.dino_patch_size)
        self.feat_type = cfg.dino_feat_type
        arch = str(cfg.model_type)
        fused = bool(getattr(cfg, "dg_fused_attention", False))
        fused_linear = bool(getattr(cfg, "dg_fused_linear", False))
        if arch not in vit.ARCHS:
            raise ValueError("Unknown arch and patch size")                     # :49-50
        kw = dict(getattr(cfg, "dg_dino_vit_kwargs", None) or {})
        if kw.pop("patch_size", self.patch_size) != self.patch_size:
            raise ValueError(f"depthg_amd: cfg.dg_dino_vit_kwargs names patch size other than cfg.dino_patch_size = {self.patch_size}")
        model = vit.ARCHS[arch](patch_size=self.patch_size, fused_attention=fused, fused_linear=fused_linear, **kw)
        path = getattr(cfg, "pretrained_weights", None)
        if path is not None:
            msg = vit.load_checkpoint(model, path)                              # :52-64
            print(f"Pretrained weights found at {path} and loaded with msg: {msg}")
        else:
            name = vit.CHECKPOINT_NAMES.get((arch, self.patch_size), f"a DINO checkpoint of {arch} with patch size {self.patch_size}")
            warnings.warn(f"depthg_amd: cfg.pretrained_weights is None - the {arch}/{self.patch_size} backbone keeps its RANDOM "
                          f"initialisation.  The reference would download {name} here; this package never does: fetch that "
                          "file yourself and name it in cfg.pretrained_weights.", stacklevel=2)
        self.model = model
        for p in self.model.parameters():                                       # :34-35
            p.requires_grad = False
        self.model.eval()
        self.n_feats = int(model.embed_dim)                                     # :70-73 (384 / 768 for ViT-S / ViT-B)
        self._register_head(dim, cfg)

    def _attn_is_read(self):
        return self.training and bool(getattr(self.cfg, "lhp", False)) and getattr(self.cfg, "propagation_strategy", "depth") == "attn"

    def _backbone(self, img, n=1, return_class_feat=False):
        """:93-120 under no_grad: (image_feat (B, C, H/p, W/p), attn) - or the class feature (B, C, 1, 1)."""
        assert img.shape[2] % self.patch_size == 0
        assert img.shape[3] % self.patch_size == 0
        if self.feat_type not in ("feat", "KK"):
            raise ValueError("Unknown feat type:{}".format(self.feat_type))     # :117
        want_attn = self._attn_is_read()
        feat, attn, qkv = self.model.get_intermediate_feat(img, n=n, want_attn=want_attn)
        feat, attn, qkv = feat[0], attn[0], qkv[0]
        B, fh, fw = feat.shape[0], img.shape[2] // self.patch_size, img.shape[3] // self.patch_size
        if return_class_feat:
            return feat[:, :1, :].reshape(B, 1, 1, -1).permute(0, 3, 1, 2), None
        if self.feat_type == "feat":
            image_feat = feat[:, 1:, :].reshape(B, fh, fw, -1).permute(0, 3, 1, 2)
        else:                                                                    # "KK": the last block's keys, heads side by side (:112-115)
            heads = qkv.shape[2]
            image_feat = qkv[1, :, :, 1:, :].reshape(B, heads, fh, fw, -1).permute(0, 1, 4, 2, 3).reshape(B, -1, fh, fw)
        if not want_attn:
            attn = torch.zeros(1, device=img.device)                            # placeholder: only `is None` is ever asked of it
        return image_feat, attn


class DinoFeaturizerWithDepth(DepthGuidance, DinoFeaturizer):
    """DinoFeaturizerWithDepth(dim, cfg) of src/modules.py:490-631 over the ViT of depthg_amd/vit.py (see the module docstring)."""

    def __init__(self, dim: int, cfg):
        super().__init__(dim, cfg)
        self._register_depth(cfg)
