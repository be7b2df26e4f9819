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
"""
import warnings

import torch
import torch.nn as nn

from . import vit
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
        (code, feats), (code_pos, feats_pos) = run_head_pair(*self._head_modules(), image_feat, image_feat_pos, True,
                                                             bool(self.cfg.dropout), float(self.dropout.p), None, defer_feats_dropout)
        return (feats, code, attn), (feats_pos, code_pos, attn_pos)


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
