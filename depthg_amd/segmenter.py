"""Producers and caller of the correlation loss: the segmentation head, the probes and one optimisation step
(SURVEY.md section 8 rows A14, N1 and the step-level caller around A13).

Mirrors, with the reference's names, parameter layout and arithmetic:
    StandInFeaturizer       DinoFeaturizer's output contract (src/modules.py:90-137: train -> (feats, code, attn), eval -> (feats,
                            code); a third Dropout2d mask on feats when cfg.dropout) over a frozen random patch embedding of the
                            ViT's geometry - the DINO weights cannot be fetched here; any module returning (B, n_feats, H/p, W/p)
                            can be passed instead.  The head (`cluster1` / `cluster2`, the three Dropout2d draws) is ONE fused HIP
                            launch (head.run_head); its registration, forward and forward_pair are
                            featurizer.FrozenBackboneFeaturizer's, shared with DinoFeaturizer (cfg.dg_dino_backbone: the real ViT).
    UnsupervisedSegmenter   LitUnsupervisedSegmenter without Lightning (src/train_segmentation.py:71-158, 169-462): the same attributes,
                            forward(x) = net(x)[1], configure_optimizers() -> three Adams, training_step (below), validation_step /
                            on_validation_epoch_end (:471-535), evaluate_batch (src/eval_segmentation.py:146-170) and segment(img),
                            the label-free route of src/demo_segmentation.py:59-78 (depthg_amd/demo.py is its command line).
                            cfg.arch == "dino_depth" (:104-106): the depth-guided featurizer, use_depth forced on.
ProjectionHead / ClusterLookup (src/modules.py:647-675) / probe_cross_entropy / fused_probe_losses live in depthg_amd/head.py and are re-exported here.

training_step is a driver over stages whose switches are all decided once, in front of the step, by training.step_plan (the featurizer
route - pair, depth or single -, whether it starts from cached features, the terms that run, this step number's histogram and
probe-reset decisions).  The stages, in the reference's order, which is the order of every launch and every random draw: zero_grad;
_refuse_or_fill;  _anchor_pass (both passes on the pair route);  LHP on the anchor code;  _positive_pass (depth and single routes);  LHP
on the positive code;  _correspondence_term (`hist/*` logs on a cfg.hist_freq step);  depth_decay.legacy_decay_step;  _auxiliary_terms
(`loss/rec`, `loss/aug_alignment`, `loss/crf`);  _probe_terms;  _backward_and_step.  The passes hand their tensors on in one record.
graph_step.GraphedTrainStep asks training.histogram_step / reset_probe_step, as the plan does, which steps it must run eagerly.
"""
from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import ops
from .aug_loss import aug_alignment_loss
from .augment import IMAGENET_MEAN, IMAGENET_STD, augment_batch, draw_augment_params
from .crf_loss import ContrastiveCRFLoss
from .depth_decay import legacy_decay_step
from .evaluation import predict_and_score, segment
from .featurizer import DepthGuidance, DinoFeaturizer, DinoFeaturizerWithDepth, FrozenBackboneFeaturizer
from .head import ClusterLookup, ProjectionHead, fused_probe_losses, probe_cross_entropy
from .lhp import LocalHiddenPositiveProjection, OriginalLocalHiddenPositiveProjection
from .loss import ContrastiveCorrelationLoss, DepthContrastiveCorrelationLoss
from .metrics import UnsupervisedMetrics
from .optim import FusedAdam, FusedAdamSet
from .parallel import GradBucket
from .rec_loss import reconstruction_loss
from .training import correspondence_total, step_plan


class StandInFeaturizer(FrozenBackboneFeaturizer):
    """DinoFeaturizer's contract with a frozen stand-in backbone (see the module docstring)."""

    def __init__(self, dim: int, cfg, backbone: Optional[nn.Module] = None):
        super().__init__()
        self.cfg, self.dim = cfg, dim
        self.patch_size = int(cfg.dino_patch_size)
        arch = str(getattr(cfg, "model_type", "vit_small"))
        self.n_feats = 384 if "small" in arch else 768          # src/modules.py:70-73
        if backbone is None:
            backbone = nn.Conv2d(3, self.n_feats, self.patch_size, stride=self.patch_size)
        self.model = backbone
        for p in self.model.parameters():                       # frozen, as the DINO ViT (:34-35)
            p.requires_grad = False
        self._register_head(dim, cfg)

    def _last_selfattention(self, img, image_feat):
        """The ViT's `get_last_selfattention` (B, heads, P+1, P+1) (src/modules.py:103-104).  A backbone that has the method is
        asked; the convolutional stand-in only builds one when the LHP module will read it (`propagation_strategy == "attn"`):
        softmax similarities of [mean token, patch tokens], channels split over 6 / 12 heads - the ViT's shapes, nothing more."""
        if hasattr(self.model, "get_last_selfattention"):
            return self.model.get_last_selfattention(img)
        if not (getattr(self.cfg, "lhp", False) and getattr(self.cfg, "propagation_strategy", "depth") == "attn"):
            return torch.zeros(1, device=image_feat.device)       # placeholder: only `is None` is ever asked of it
        b, c, h, w = image_feat.shape
        heads = 6 if self.n_feats == 384 else 12
        tok = image_feat.flatten(2).transpose(1, 2)                                   # (B,P,C)
        tok = torch.cat([tok.mean(1, keepdim=True), tok], dim=1).reshape(b, h * w + 1, heads, c // heads).transpose(1, 2)
        return torch.softmax(tok @ tok.transpose(-1, -2) / (c // heads) ** 0.5, dim=-1)

    def _backbone(self, img, n=1, return_class_feat=False):
        assert img.shape[2] % self.patch_size == 0 and img.shape[3] % self.patch_size == 0   # :93-94
        image_feat = self.model(img)
        if return_class_feat:
            return image_feat.mean((2, 3), keepdim=True), None
        return image_feat, self._last_selfattention(img, image_feat)


class StandInFeaturizerWithDepth(DepthGuidance, StandInFeaturizer):
    """DinoFeaturizerWithDepth's contract (src/modules.py:490-631; featurizer.DepthGuidance) over the frozen stand-in backbone."""

    def __init__(self, dim: int, cfg, backbone: Optional[nn.Module] = None):
        super().__init__(dim, cfg, backbone)
        self._register_depth(cfg)


class UnsupervisedSegmenter(nn.Module):
    """LitUnsupervisedSegmenter(n_classes, cfg) without the Lightning plumbing (src/train_segmentation.py:71-158)."""

    def __init__(self, n_classes: int, cfg, net: Optional[nn.Module] = None):
        super().__init__()
        self.cfg, self.n_classes = cfg, n_classes
        dim = n_classes if not cfg.continuous else cfg.dim                          # :78-81
        self.use_depth = bool(cfg.use_depth)
        self.depth_arch = getattr(cfg, "arch", "dino") == "dino_depth"
        if self.depth_arch:
            self._refuse_depth_arch_combinations(cfg)
        if getattr(cfg, "dg_feature_cache", None) and getattr(cfg, "lhp", False) and getattr(cfg, "propagation_strategy", "depth") == "attn":
            raise ValueError("depthg_amd: cfg.dg_feature_cache cannot be combined with cfg.lhp under propagation_strategy = 'attn': the "
                             "cache keeps image_feat, not the last block's attention map the LHP module would read")
        if getattr(cfg, "dg_val_feature_cache", None):
            self._refuse_val_feature_cache_combinations(cfg)
        if net is None:                                                               # :99-108
            # cfg.dg_dino_backbone (build-side key, off by default): the real DINO ViT (featurizer.DinoFeaturizer) instead of the stand-in
            real = getattr(cfg, "dg_dino_backbone", False)
            if self.depth_arch:                                                       # :104-106 (arch == "dino_depth")
                net = DinoFeaturizerWithDepth(dim, cfg) if real else StandInFeaturizerWithDepth(dim, cfg)
            else:                                                                     # (arch == "dino", any other value, or no key)
                net = DinoFeaturizer(dim, cfg) if real else StandInFeaturizer(dim, cfg)
        if self.depth_arch:
            self.use_depth = True                                                     # :106
        self.net = net
        self.train_cluster_probe = ClusterLookup(dim, n_classes)                      # :110
        self.cluster_probe = ClusterLookup(dim, n_classes + cfg.extra_clusters)       # :112
        self.linear_probe = nn.Conv2d(dim, n_classes, (1, 1))                         # :113
        self.cluster_metrics = UnsupervisedMetrics("test/cluster/", n_classes, cfg.extra_clusters, True)      # :117-125
        self.linear_metrics = UnsupervisedMetrics("test/linear/", n_classes, 0, False)
        self.test_cluster_metrics = UnsupervisedMetrics("final/cluster/", n_classes, cfg.extra_clusters, True)
        self.test_linear_metrics = UnsupervisedMetrics("final/linear/", n_classes, 0, False)
        self.linear_probe_loss_fn = nn.CrossEntropyLoss()                             # :127 (kept for the surface; the step uses the fused HIP loss)
        # :128-129; the reference's defaults (src/configs/train_config.yml) where a configuration lacks the keys
        self.crf_loss_fn = ContrastiveCRFLoss(getattr(cfg, "crf_samples", 1000), getattr(cfg, "alpha", .5), getattr(cfg, "beta", .15),
                                              getattr(cfg, "gamma", .05), getattr(cfg, "w1", 10.0), getattr(cfg, "w2", 3.0),
                                              getattr(cfg, "shift", 0.0))
        # :79, :133-134: cfg.use_depth_only_intra swaps in DepthContrastiveCorrelationLoss, whose intra pair-set correlates the
        # depth-augmented features; absent or False: the class, draws and launches are what they were
        self.depth_only_intra = bool(getattr(cfg, "use_depth_only_intra", False))
        if self.depth_only_intra:
            self._refuse_depth_only_intra_combinations(cfg)
            self.contrastive_corr_loss_fn = DepthContrastiveCorrelationLoss(cfg)
        else:
            self.contrastive_corr_loss_fn = ContrastiveCorrelationLoss(cfg)           # :131 (shares cfg: the decay below mutates it)
        for p in self.contrastive_corr_loss_fn.parameters():                          # :136
            p.requires_grad = False
        if getattr(cfg, "lhp", False):                                                 # :82-87
            original = "lhp_original" in str(getattr(cfg, "experiment_name", ""))
            self.lhp_module = OriginalLocalHiddenPositiveProjection(cfg) if original else LocalHiddenPositiveProjection(cfg)
        # cfg.dg_fused_probes (build-side key, absent or False by default): _probe_terms makes ONE call, head.fused_probe_losses, on
        # the detached code instead of the convolution and the two probe operations.  Read here, once: the step's plan does not carry it.
        self.fused_probes = bool(getattr(cfg, "dg_fused_probes", False))
        self.automatic_optimization = False                                           # :139
        self.global_step = 0
        self._optims = None
        self.validation_step_outputs = []                                             # :149-157
        self.max_cluster_accuracy = self.max_cluster_miou = self.max_linear_accuracy = self.max_linear_miou = 0.0
        # :115 - the reconstruction term's decoder.  The reference always builds it and steps it only under rec_weight (:540-541);
        # here it exists only then, and is built LAST: with rec_weight = 0 no module, no state_dict key and no random draw is
        # added, and with it on every other module still takes the draws it takes without it - no existing initial value moves.
        if getattr(cfg, "rec_weight", 0) > 0:
            self.decoder = nn.Conv2d(dim, self.net.n_feats, (1, 1))

    @staticmethod
    def _refuse_depth_arch_combinations(cfg):
        """cfg.arch == "dino_depth" with a term that cannot run on it (asked at construction and again in front of a step's first launch)."""
        if getattr(cfg, "aug_alignment_weight", 0) > 0:
            raise ValueError("depthg_amd: cfg.aug_alignment_weight > 0 cannot be combined with cfg.arch = 'dino_depth': the term's third "
                             "featurizer pass has no depth map (the reference's `self.net(img_aug)` fails the depth featurizer's "
                             "two-tuple assertion, src/modules.py:609)")
        if getattr(cfg, "rec_weight", 0) > 0 and getattr(cfg, "guidance", "none") in ("sum", "cross_attn") \
                and not getattr(cfg, "dg_rec_feats_grad", False):
            raise ValueError(f"depthg_amd: cfg.rec_weight > 0 cannot be combined with cfg.arch = 'dino_depth' under guidance "
                             f"{cfg.guidance!r}: there feats depend on trainable depth modules and the fused reconstruction kernels "
                             "have no gradient with respect to feats, unless cfg.dg_rec_feats_grad = True asks them for it")

    @staticmethod
    def _refuse_depth_only_intra_combinations(cfg):
        """cfg.use_depth_only_intra with a configuration its loss cannot run on (asked at construction and in front of a step)."""
        if getattr(cfg, "arch", "dino") != "dino_depth":
            raise ValueError(f"depthg_amd: cfg.use_depth_only_intra needs cfg.arch = 'dino_depth': under arch "
                             f"{getattr(cfg, 'arch', 'dino')!r} (\"dino\") the featurizer produces no depth-augmented features for the "
                             "intra pair-set to correlate")
        if getattr(cfg, "lhp", False):
            raise ValueError("depthg_amd: cfg.use_depth_only_intra cannot be combined with cfg.lhp (the second loss call on the "
                             "projected code is not built for DepthContrastiveCorrelationLoss); set cfg.lhp = False")
        if getattr(cfg, "depth_feat_correlation_loss", False):
            raise ValueError("depthg_amd: cfg.use_depth_only_intra cannot be combined with cfg.depth_feat_correlation_loss: "
                             "DepthContrastiveCorrelationLoss returns six values and has no depth term; set "
                             "cfg.depth_feat_correlation_loss = False")

    @staticmethod
    def _refuse_true_labels_combinations(cfg, batch):
        """cfg.use_true_labels with a batch or a configuration its signal cannot be formed for (asked in front of a step's first launch)."""
        if "label_pos" not in batch:
            raise KeyError("training_step: cfg.use_true_labels needs batch['label_pos'] (the positive image's labels are its signal, "
                           "src/train_segmentation.py:219-225); use a dataset that hands them out (data.ContrastiveBatches does) or set "
                           "cfg.use_true_labels = False")
        if getattr(cfg, "use_depth_only_intra", False):
            raise ValueError("depthg_amd: cfg.use_true_labels cannot be combined with cfg.use_depth_only_intra: DepthContrastiveCorrelationLoss "
                             "correlates the backbone's and the depth-augmented features, and the one-hot labels would replace only one of "
                             "them; set one of the two keys to False")

    def forward(self, x):
        return self.net(x)[1]                                                          # :160-167

    def configure_optimizers(self):                                                    # :537-547
        # as the reference: net_optim steps `self.net.parameters()` (the head; with the depth-guided featurizer also the depth modules
        # its guidance trains - the rest of the net has requires_grad = False) and, when the reconstruction term is on (rec_weight > 0,
        # :540-541), its decoder's (the CRF and augmentation-alignment terms have no parameters of their own) - the LHP projection
        # head is NOT among them, so it keeps its initial weights there and here
        main_params = list(self.net.parameters()) + self._decoder_parameters()
        # (cfg.dg_fused_adam: the same three as optim.FusedAdam, stepped by one HIP launch - optim.FusedAdamSet)
        adam = FusedAdam if getattr(self.cfg, "dg_fused_adam", False) else torch.optim.Adam
        return (adam([p for p in main_params if p.requires_grad], lr=self.cfg.lr),                    # net, linear probe, cluster probe
                adam(list(self.linear_probe.parameters()), lr=5e-3), adam(list(self.cluster_probe.parameters()), lr=5e-3))

    def optimizers(self):
        if self._optims is None:
            self._optims = self.configure_optimizers()
        return self._optims

    def _fused_set(self):
        """cfg.dg_fused_adam: the three optimisers as one FusedAdamSet (rebuilt when `_optims` is replaced)."""
        optims = self.optimizers()
        cached = getattr(self, "_optim_set", None)
        if cached is None or cached[0] is not optims:
            self._optim_set = cached = (optims, FusedAdamSet(optims))
        return cached[1]

    def _handed_over_grads(self, handed, fused):
        """What `grad_sync` returned -> the `grads` of FusedAdamSet.step, or None (read p.grad)."""
        if not isinstance(handed, (GradBucket, list)):
            return None
        if not fused:
            raise RuntimeError("training_step: `grad_sync` handed gradients over, which only the fused optimiser step reads "
                               "(cfg.dg_fused_adam); without it unpack the bucket into p.grad and return None")
        params = fused.parameters()
        if isinstance(handed, GradBucket):
            views = {id(p): v for p, v in zip(handed.parameters(), handed.grad_views())}
            missing = [tuple(p.shape) for p in params if id(p) not in views]
            if missing:
                raise RuntimeError(f"training_step: the GradBucket lacks stepped parameters of shapes {missing} "
                                   "(build it from all_reduced_parameters())")
            return [views[id(p)] for p in params]
        if len(handed) != len(params):
            raise RuntimeError(f"training_step: `grad_sync` returned {len(handed)} gradients for {len(params)} stepped parameters")
        return handed

    def _decoder_parameters(self):
        """The reconstruction term's decoder (weight, bias) when cfg.rec_weight > 0 built one, else nothing."""
        decoder = getattr(self, "decoder", None)
        return list(decoder.parameters()) if decoder is not None and getattr(self.cfg, "rec_weight", 0) > 0 else []

    def head_parameters(self):
        """The parameters of the featurizer net_optim steps: cluster1 + cluster2 and, under cfg.arch
        "dino_depth", the depth modules cfg.guidance trains (the others are built with requires_grad = False)."""
        return [p for p in self.net.parameters() if p.requires_grad]

    def all_reduced_parameters(self):
        """Every parameter one of the three optimisers steps - the head, under cfg.arch "dino_depth" the trained depth modules and,
        under cfg.rec_weight, the decoder (net_optim), the linear probe and the cluster probe, in the optimisers' order.
        Under data parallelism ALL of them must be averaged over the ranks before the optimiser steps (build the GradBucket
        from this list), or the replicas' probes drift apart.  (The LHP head is stepped by no optimiser, as in the reference,
        src/train_segmentation.py:537-547, so it needs no exchange.)"""
        return self.head_parameters() + self._decoder_parameters() + list(self.linear_probe.parameters()) + \
            list(self.cluster_probe.parameters())

    def training_step(self, batch: Dict[str, torch.Tensor], batch_idx: int = 0, grad_sync=None):
        """One optimisation step (src/train_segmentation.py:169-462); returns (loss, logs).  `grad_sync`: callable run between backward and
        the optimiser steps (data parallelism: GradBucket pack / all-reduce / unpack).  With cfg.dg_fused_adam it may hand the averaged
        gradients straight to the optimiser step instead of unpacking them into p.grad: it returns the `GradBucket` (its `grad_views()` are
        read, matched to the parameters by identity), or a `list` of tensors / None aligned with `all_reduced_parameters()`, e.g.
            grad_sync = lambda: [bucket.pack(), bucket.allreduce_mean_(), bucket][-1]
        Any other return value - None, or the tuple a `lambda: (a(), b())` chain yields - keeps today's meaning: p.grad is read."""
        plan = step_plan(self.cfg, net=self.net, batch=batch, depth_arch=self.depth_arch, depth_only_intra=self.depth_only_intra,
                         global_step=self.global_step)
        for optim in self.optimizers():                                                               # :174-176
            optim.zero_grad()
        img, label = batch["img"], batch["label"]
        depth, depth_pos = (batch["depth"], batch["depth_pos"]) if self.use_depth else (None, None)
        batch = self._refuse_or_fill(plan, batch)
        p = self._anchor_pass(plan, batch, depth)
        lhp_code = self.lhp_module(p.code, depth, img, p.attn) if plan.lhp else None                  # :202-203
        logs, loss = {}, 0
        if plan.correspondence:
            # (the positive pass stays behind the LHP call above: that module draws random numbers)
            self._positive_pass(plan, batch, depth_pos, p)
            lhp_code_pos = self.lhp_module(p.code_pos, None) if plan.lhp else None                    # :214-215
            total, logs = self._correspondence_term(plan, batch, p, (depth, depth_pos), (lhp_code, lhp_code_pos))
            loss = loss + total
        # the legacy decays sit at function-body level in the reference: they run every step, whatever correspondence_weight is
        legacy_decay_step(self.cfg, self.contrastive_corr_loss_fn.cfg, self.global_step)             # :356-375 (mutates cfg)
        loss = self._auxiliary_terms(plan, batch, p, loss, logs)
        loss = self._probe_terms(p.code, label, loss, logs)
        self._backward_and_step(plan, loss, grad_sync)
        return loss.detach(), logs

    def _refuse_or_fill(self, plan, batch):
        """What can refuse the step, asked before anything is launched (cfg may have changed since construction) -> the batch to read."""
        if self.depth_arch:
            self._refuse_depth_arch_combinations(self.cfg)
        if self.depth_only_intra:
            self._refuse_depth_only_intra_combinations(self.cfg)
        if getattr(self.cfg, "use_true_labels", False):
            self._refuse_true_labels_combinations(self.cfg, batch)
        if not plan.aug:
            return batch
        # cfg.dg_gpu_augment (build-side key, absent or False by default): a batch without the augmented view gets it here - parameters drawn
        # from torch's global CPU generator (host work: such a step is not captured into a graph), both tensors from batch["img"] at its own
        # size in two HIP launches (augment.augment_batch).  "unit": img is ImageNet-normalised and the colour ops work on [0, 1] values; any
        # other true value: the ops act on the tensor as given, as the reference's do.  A batch that carries the keys wins, untouched.
        if plan.gpu_augment and "img_aug" not in batch:
            img, unit = batch["img"], plan.gpu_augment == "unit"
            params = draw_augment_params(img.shape[0], img.shape[2], img.shape[3])
            img_aug, coord_aug = augment_batch(img, params, mean=IMAGENET_MEAN if unit else None, std=IMAGENET_STD if unit else None)
            batch = {**batch, "img_aug": img_aug, "coord_aug": coord_aug}
        for key in ("img_aug", "coord_aug"):
            if key not in batch:
                raise KeyError(f"training_step: cfg.aug_alignment_weight = {self.cfg.aug_alignment_weight} needs batch[{key!r}] "
                               "(the dataset's augmented view and its coordinate map, src/data.py:1132-1139)")
        return batch

    def _anchor_pass(self, plan, batch, depth):
        """The featurizer pass on the anchor image - on the pair route both passes at once - as one record.  plan.cached
        (cfg.dg_feature_cache, build-side key, absent or None by default): the batch carries `image_feat` / `image_feat_pos` - the frozen
        backbone's outputs, kept by feature_cache.FeatureCache and gathered by data.ContrastiveBatches - and the pass starts behind the
        backbone; the head's draws and launches are unchanged.  (The augmentation-alignment term's third pass still runs the backbone.)"""
        # (the record the later stages read - image_feat: the depth route's third output; rec_feats: this pass's ATTACHED feats)
        p = SimpleNamespace(feats=None, code=None, attn=None, image_feat=None, feats_pos=None, code_pos=None, image_feat_pos=None, rec_feats=None)
        net, img = self.net, batch["img"]
        if plan.route == "pair":
            # (on the dense identity grid the Dropout2d of the returned feats is applied by the loss's operand preparation: the
            #  dropped feature tensors are never written - ops.DeferredDropout)
            ps = getattr(net, "patch_size", None)
            defer = ps is not None and getattr(net, "supports_deferred_dropout", False) and \
                self.contrastive_corr_loss_fn.takes_deferred_dropout((img.shape[2] // ps, img.shape[3] // ps))
            (p.feats, p.code, p.attn), (p.feats_pos, p.code_pos, _) = \
                net.forward_pair_features(batch["image_feat"], batch["image_feat_pos"], defer) if plan.cached else \
                net.forward_pair(img, batch["img_pos"], defer) if defer else net.forward_pair(img, batch["img_pos"])   # :194-200, :207-212
        elif plan.route == "depth":
            # (feats carry a graph under guidance "sum" / "cross_attn"; the correlation loss reads them under no_grad, src/modules.py:1232-1234)
            feats, p.code, p.image_feat, p.attn = net((img, depth))                                  # :191-197
            # (cfg.dg_rec_feats_grad: the reconstruction term reads the attached tensor, :391-398, and trains the depth modules through it)
            p.rec_feats = feats if plan.rec_feats_grad and plan.rec and feats.requires_grad else None
            p.feats = feats.detach()
        elif plan.cached:
            p.feats, p.code, p.attn = net.forward_features(batch["image_feat"])
        else:
            p.feats, p.code, p.attn = net(img)                                                       # :194-200
        if plan.cached and p.attn is None and plan.lhp:
            # (the LHP module projects without propagating when `attn is None`, :191-192; the featurizers hand it a placeholder where
            #  nothing reads the map - so does the cached pass: the "attn" strategy, which would read it, is refused at construction)
            p.attn = torch.zeros(1, device=p.code.device)
        return p

    def _positive_pass(self, plan, batch, depth_pos, p):
        """The featurizer pass on the positive image, where the anchor pass did not run it (the depth and single routes)."""
        if plan.route == "depth":
            feats_pos, p.code_pos, p.image_feat_pos, _ = self.net((batch["img_pos"], depth_pos))     # :205-210
            p.feats_pos = feats_pos.detach()
        elif plan.route == "single":
            p.feats_pos, p.code_pos, _ = self.net.forward_features(batch["image_feat_pos"]) if plan.cached else \
                self.net(batch["img_pos"])                                                           # :207-212

    def _correspondence_term(self, plan, batch, p, depths, lhp_codes):
        """The correlation loss, its histograms, its second call on the LHP codes and the weighted total (:229-350) -> (term, logs)."""
        loss_fn = self.contrastive_corr_loss_fn
        salience = batch["mask"].to(torch.float32).squeeze(1) if plan.use_salience else None         # :233-238
        salience_pos = batch["mask_pos"].to(torch.float32).squeeze(1) if plan.use_salience else None
        d_args = depths if plan.depth_term else (None, None)                                         # :242-292
        signal, signal_pos = p.feats, p.feats_pos
        if plan.depth_only_intra:
            # :240-350 with the class of :133-134.  The reference's own call passes `depth=` / `depth_pos=` to parameters named
            # depth_aug_feats / depth_aug_feats_pos and raises a TypeError; this is the call the names ask for: the frozen
            # backbone's features (the featurizer's third output) as orig_feats, the depth-augmented ones (its first) as depth_aug_feats
            out = loss_fn(p.image_feat.detach(), p.image_feat_pos.detach(), salience, salience_pos, p.code, p.code_pos, p.feats, p.feats_pos)
        else:
            if getattr(self.cfg, "use_true_labels", False):
                # :219-225: the one-hot ground-truth labels replace the frozen backbone's features as the loss's signal - the method's
                # supervised upper bound; everything else in the step is unchanged.  Both maps from one HIP launch, at the labels' own
                # resolution (ops.label_onehot; under cfg.dg_graph_safe without the host's look at the labels' range).  Read here: the
                # step's plan does not carry the key.  Absent or False: nothing of this runs.
                signal, signal_pos = ops.label_onehot(batch["label"], self.n_classes, batch["label_pos"],
                                                      check=not getattr(self.cfg, "dg_graph_safe", False))
            out = loss_fn(signal, signal_pos, salience, salience_pos, p.code, p.code_pos, *d_args)
        # :229-231, :298-301: every cfg.hist_freq steps the reference histograms the three un-reduced cd tensors - here one small
        # launch on the operands this call left in its workspace (in front of the LHP call, which runs the loss again)
        hists = loss_fn.cd_histograms(bins=plan.hist_bins) if plan.histograms else None
        lhp_out = loss_fn(signal, signal_pos, salience, salience_pos, *lhp_codes, *d_args) if plan.lhp and plan.depth_term else None
        total, logs = correspondence_total(self.cfg, out, lhp_out)                                   # :303-350
        if hists is not None:
            logs.update({"hist/" + k: v for k, v in hists.items()})
        return total, logs

    def _auxiliary_terms(self, plan, batch, p, loss, logs):
        """The reconstruction, augmentation-alignment and CRF terms, in the reference's order; each logs itself.  Returns the loss."""
        cfg = self.cfg
        # :391-398: the reconstruction term - the decoder's 1 x 1 convolution of code against feats, both normalised - as one fused
        # HIP forward and one HIP backward (rec_loss.reconstruction_loss): rec_feats is never written.  feats goes in as it is: in
        # the paired pass it may be an ops.DeferredDropout, whose mask the kernels apply.  Off: nothing is launched or logged.
        if plan.rec:
            if getattr(self, "decoder", None) is None:
                raise RuntimeError(f"training_step: cfg.rec_weight = {cfg.rec_weight} but this segmenter was built without a decoder "
                                   "(rec_weight was 0 then); set cfg.rec_weight before constructing UnsupervisedSegmenter")
            if p.rec_feats is not None:  # (arch "dino_depth" under "sum" / "cross_attn" with cfg.dg_rec_feats_grad: d feats is written too)
                rec = reconstruction_loss(p.code, p.rec_feats, self.decoder.weight, self.decoder.bias, feats_grad=True)
            else:
                rec = reconstruction_loss(p.code, p.feats, self.decoder.weight, self.decoder.bias)
            logs["loss/rec"] = rec.detach()
            loss = loss + cfg.rec_weight * rec
        # :400-411: the augmentation-alignment term - a third featurizer pass (in training mode: its own Dropout2d draws, as the
        # reference's would be) and aug_loss.aug_alignment_loss, one fused HIP forward and one HIP backward whose gradient reaches the
        # head through both maps.  (:401 unpacks two values where the training-mode featurizer returns three: the intent is element 1.)
        # Off: no pass, no draw, no launch, and the batch may lack the two keys.
        if plan.aug:
            code_aug = self.net(batch["img_aug"])[1]
            aug_alignment = aug_alignment_loss(p.code, code_aug, batch["coord_aug"])
            logs["loss/aug_alignment"] = aug_alignment.detach()
            loss = loss + cfg.aug_alignment_weight * aug_alignment
        # :413-419: the contrastive CRF term, one fused HIP forward (the maps are resized at the crf_samples positions only, the
        # similarity kernel is formed on the fly) and one HIP backward - ContrastiveCRFLoss.mean_loss.  Off: nothing is drawn or launched.
        if plan.crf:
            crf = self.crf_loss_fn.mean_loss(batch["img"], p.code)
            logs["loss/crf"] = crf.detach()
            loss = loss + cfg.crf_weight * crf
        return loss

    def _probe_terms(self, code, label, loss, logs):
        """The probes on the detached code (:421-444); logs both terms and the total.  Returns the loss."""
        if self.fused_probes:
            # both probes, and already their parameter gradients, in one HIP forward (no clone: the operation only reads the code)
            linear_loss, cluster_loss = fused_probe_losses(code.detach(), label, self.linear_probe.weight, self.linear_probe.bias,
                                                           self.cluster_probe.clusters)
            loss = loss + linear_loss + cluster_loss
            logs.update({"loss/linear": linear_loss.detach(), "loss/cluster": cluster_loss.detach(), "loss/total": loss.detach()})
            return loss
        detached_code = code.detach().clone()
        # resize to the label resolution + masked cross entropy in one HIP kernel (the reference materialises the logits at label
        # resolution and three masks, :427-434); the cluster probe's similarity / arg-max / loss likewise
        linear_loss = probe_cross_entropy(self.linear_probe(detached_code), label)
        cluster_loss, _ = self.cluster_probe(detached_code, None)
        loss = loss + linear_loss + cluster_loss
        logs.update({"loss/linear": linear_loss.detach(), "loss/cluster": cluster_loss.detach(), "loss/total": loss.detach()})
        return loss

    def _backward_and_step(self, plan, loss, grad_sync):
        """Backward, `grad_sync`, the optimiser step or steps, the probe reset on its step, the step count (:446-455)."""
        net_optim, linear_probe_optim, cluster_probe_optim = self.optimizers()
        loss.backward()                                                                               # :446
        fused = self._fused_set() if plan.fused_adam else None
        grads = self._handed_over_grads(grad_sync() if grad_sync is not None else None, fused)
        if fused is not None:
            fused.step(grads=grads)                                                                   # :447-449 in one HIP launch
        else:
            net_optim.step(); cluster_probe_optim.step(); linear_probe_optim.step()                   # :447-449
        if plan.reset_probes:                                                                         # :451-455
            self.linear_probe.reset_parameters()
            self.cluster_probe.reset_parameters()
            adam = FusedAdam if fused is not None else torch.optim.Adam
            self._optims = (net_optim, adam(list(self.linear_probe.parameters()), lr=5e-3),
                            adam(list(self.cluster_probe.parameters()), lr=5e-3))
        self.global_step += 1

    @staticmethod
    def _refuse_val_feature_cache_combinations(cfg):
        """cfg.dg_val_feature_cache with a configuration whose evaluation cannot start behind the backbone (asked at construction)."""
        from .feature_cache import as_dtype
        as_dtype(cfg.dg_val_feature_cache)
        if getattr(cfg, "arch", "dino") == "dino_depth":
            raise ValueError("depthg_amd: cfg.dg_val_feature_cache serves cfg.arch = 'dino': the evaluation branch of the depth-guided "
                             "featurizer (arch 'dino_depth') forms its features from the image and has no forward_features; leave "
                             "cfg.dg_val_feature_cache unset (validation then runs the backbone) or use arch 'dino'")

    def _cached_eval_features(self, batch, flip):
        """(image_feat, image_feat_flip) for the evaluation routes to start from, or (None, None): the backbone runs.  Only with
        cfg.dg_val_feature_cache (build-side key, absent or None by default) and a batch that carries `image_feat` - the frozen
        backbone's output on batch["img"], kept by a feature_cache.FeatureCache of the split (train.val_feature_cache) and gathered
        by data.ContrastiveBatches(pos=False, feature_cache=...); `image_feat_flip`: the same of the mirrored images, from a second
        cache (data.build_feature_cache(mirrored=True))."""
        if not getattr(self.cfg, "dg_val_feature_cache", None) or "image_feat" not in batch:
            return None, None
        img, feats = batch["img"], [batch["image_feat"]]
        if flip:
            if "image_feat_flip" not in batch:
                raise ValueError("depthg_amd: evaluate_batch(flip=True) from cached features needs batch['image_feat_flip'] as well: "
                                 "the backbone's features of the MIRRORED images (a mirrored feature map is not the feature map of "
                                 "the mirrored image: the ViT's position embedding is not symmetric).  Build a second cache with "
                                 "data.build_feature_cache(..., mirrored=True) and gather it into the batch, call "
                                 "evaluate_batch(flip=False), or drop 'image_feat' from the batch to run the backbone")
            feats.append(batch["image_feat_flip"])
        if self.depth_arch or not all(hasattr(self.net, a) for a in ("forward_features", "patch_size", "n_feats")):
            raise ValueError("depthg_amd: cfg.dg_val_feature_cache needs a featurizer with a pass from cached features "
                             "(FrozenBackboneFeaturizer.forward_features, cfg.arch = 'dino'); leave the key unset to run the backbone")
        ps = int(self.net.patch_size)
        want = (img.shape[0], int(self.net.n_feats), img.shape[2] // ps, img.shape[3] // ps)
        for name, f in zip(("image_feat", "image_feat_flip"), feats):
            if f.dim() != 4 or tuple(f.shape) != want:
                raise ValueError(f"depthg_amd: batch[{name!r}] is {tuple(f.shape)}, the featurizer's output on images of "
                                 f"{tuple(img.shape)} is {want}: the cache was built for another backbone or resolution - rebuild it "
                                 "(train.val_feature_cache at this eval_res) or leave cfg.dg_val_feature_cache unset")
        return feats[0], (feats[1] if flip else None)

    def _eval_mode_codes(self, img, flip, image_feat=None, image_feat_flip=None):
        """code = net(img)[1] (and of the mirrored images when `flip`) with the net in eval mode; the net's mode is restored after
        (what Lightning does around its validation loop: the next training_step needs the training-mode 3-tuple).  With `image_feat`
        (and, under `flip`, `image_feat_flip`: the backbone's features of the mirrored images) the pass starts behind the backbone:
        code = net.forward_features(image_feat)[1], the eval-mode head - no dropout, no draw."""
        if image_feat is not None and flip and image_feat_flip is None:
            raise ValueError("depthg_amd: the flipped pass from cached features needs image_feat_flip (data.build_feature_cache(..., "
                             "mirrored=True)): a mirrored feature map is not the feature map of the mirrored image")
        was_training = self.net.training
        self.net.eval()
        try:
            with torch.no_grad():
                if image_feat is not None:
                    code = self.net.forward_features(image_feat)[1]
                    code_flip = self.net.forward_features(image_feat_flip)[1] if flip else None
                else:
                    code = self.net(img)[1]
                    code_flip = self.net(img.flip(dims=[3]))[1] if flip else None
        finally:
            self.net.train(was_training)
        return code, code_flip

    def validation_step(self, batch: Dict[str, torch.Tensor], batch_idx: int = 0):
        """src/train_segmentation.py:471-499: the probes' arg-max predictions at the label resolution into linear_metrics /
        cluster_metrics, one HIP launch pair (evaluation.predict_and_score) instead of the resize, 1x1 convolution, cosine
        similarities and bincounts at label resolution.  Appends and returns the first cfg.n_images of img, linear_preds,
        cluster_preds and label, on the CPU.  With cfg.dg_val_feature_cache set, a batch that carries `image_feat` skips the
        backbone (the batch keeps `img`: it is returned); a batch without the key, or any batch without the cfg key, runs it."""
        img, label = batch["img"], batch["label"]
        k = int(getattr(self.cfg, "n_images", 5))
        # cfg.dg_val_feature_cache and a batch with `image_feat`: the pass starts behind the frozen backbone (_cached_eval_features)
        code, _ = self._eval_mode_codes(img, False, *self._cached_eval_features(batch, False))
        linear_preds, cluster_preds = predict_and_score(code, label, self.linear_probe, self.cluster_probe, self.linear_metrics,
                                                        self.cluster_metrics, n_store=k)
        none = torch.empty((0,) + tuple(label.shape[-2:]), dtype=torch.int64)          # (n_images = 0)
        out = {"img": img[:k].detach().cpu(),
               "linear_preds": linear_preds.cpu() if linear_preds is not None else none,
               "cluster_preds": cluster_preds.cpu() if cluster_preds is not None else none.clone(),
               "label": label[:k].detach().cpu()}
        self.validation_step_outputs.append(out)
        return out

    def on_validation_epoch_end(self) -> Dict[str, float]:
        """src/train_segmentation.py:501-535 without the logger: both metrics, the running maxima, reset; returns the metrics."""
        tb_metrics = {**self.linear_metrics.compute(), **self.cluster_metrics.compute()}
        for prefix, metric, attr in (("test/cluster/", "Accuracy", "max_cluster_accuracy"), ("test/cluster/", "mIoU", "max_cluster_miou"),
                                     ("test/linear/", "Accuracy", "max_linear_accuracy"), ("test/linear/", "mIoU", "max_linear_miou")):
            setattr(self, attr, max(getattr(self, attr), tb_metrics[prefix + metric]))
            tb_metrics[prefix + "Max" + metric] = getattr(self, attr)        # (new keys: appended behind the metrics, in this order)
        self.linear_metrics.reset()
        self.cluster_metrics.reset()
        self.validation_step_outputs.clear()
        return tb_metrics

    def evaluate_batch(self, batch: Dict[str, torch.Tensor], flip: bool = True, run_crf: bool = False):
        """src/eval_segmentation.py:146-170: code of the image and (flip) of its mirror, averaged as (code1 + code2.flip(3)) / 2
        inside the projection, the probes' arg-max predictions into test_linear_metrics / test_cluster_metrics; with run_crf
        (eval_config.yml's run_crf) both probes' outputs are refined by the dense CRF on the batch's images first (:162-167).
        Returns (linear_preds, cluster_preds) (B,H,W) int64 on the GPU.  With cfg.dg_val_feature_cache set, a batch that carries
        `image_feat` and (flip) `image_feat_flip` - the backbone's features of the mirrored images, from a cache built with
        data.build_feature_cache(mirrored=True) - skips the backbone; `image_feat` alone under flip is refused."""
        img, label = batch["img"], batch["label"]
        code, code_flip = self._eval_mode_codes(img, flip, *self._cached_eval_features(batch, flip))
        return predict_and_score(code, label, self.linear_probe, self.cluster_probe, self.test_linear_metrics,
                                 self.test_cluster_metrics, code_flip=code_flip, n_store=img.shape[0], img=img if run_crf else None,
                                 run_crf=run_crf)

    def segment(self, img: torch.Tensor, flip: bool = True, run_crf: bool = False, overlay: Optional[float] = None, remap: bool = True):
        """Label-free inference on normalised images (B,3,H,W) (src/demo_segmentation.py:59-78): the codes as evaluate_batch forms
        them (eval mode, no_grad; `flip`: averaged with the mirrored pass), then evaluation.segment at the images' own size - byte
        label maps of both probes and, with `overlay` (the colours' weight in [0, 1]), painted images; `run_crf` refines with the
        dense CRF first.  `remap`: the cluster ids go through the Hungarian assignment of test_cluster_metrics if its compute() has
        run, else of cluster_metrics, else (or with remap=False) they stay raw as in the reference demo.  Returns evaluation.Segmentation."""
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"depthg_amd: segment takes normalised images (B, 3, H, W), got {tuple(img.shape)}")
        metrics = None
        if remap:
            metrics = next((mt for mt in (self.test_cluster_metrics, self.cluster_metrics) if getattr(mt, "assignments", None) is not None), None)
        code, code_flip = self._eval_mode_codes(img, flip)
        return segment(code, img.shape[-2:], self.linear_probe, self.cluster_probe, code_flip=code_flip, cluster_metrics=metrics,
                       run_crf=run_crf, img=img if (run_crf or overlay is not None) else None, overlay=overlay)


def default_segmenter_cfg(**over) -> SimpleNamespace:
    """The keys training_step and the featurizer read, with the values of src/configs/local_config.yml."""
    cfg = SimpleNamespace(
        # featurizer / head
        model_type="vit_small", dino_patch_size=8, dino_feat_type="feat", projection_type="nonlinear", dropout=True,
        pretrained_weights=None, continuous=True, dim=70, extra_clusters=0, arch="dino", lr=5e-4, reset_probe_steps=None,
        # loss (hot path)
        feature_samples=11, use_salience=False, depth_sampling="fps", fps_gpu=False, pointwise=True, zero_clamp=True, stabalize=False,
        pos_intra_shift=0.18, pos_inter_shift=0.12, neg_inter_shift=0.46, neg_samples=5,
        depth_feat_correlation_loss=True, depth_feat_shift=0.03,
        # caller
        use_depth=True, use_true_labels=False, correspondence_weight=1.0, pos_inter_weight=0.25, pos_intra_weight=0.67,
        neg_inter_weight=0.63, depth_feat_weight=0.19, rec_weight=0.0, aug_alignment_weight=0.0, crf_weight=0.0, hist_freq=100,
        depth_loss_decay=True, depth_loss_decay_factor=0.6, decay_every_steps=250, fix_depth_feat_shift=False,
        fps_until_step=0, post_fps_samples=11, fps_sample_decay=True, fps_sample_decay_every_steps=1000,
        fps_sample_decay_factor=0.9, fps_min_samples=0, lhp=False, lhp_weight=0.2, lhp_weight_balance=False,
        lhp_depth_weight=0.5,
        # the contrastive CRF term (crf_weight > 0): ContrastiveCRFLoss(crf_samples, alpha, beta, gamma, w1, w2, shift)
        crf_samples=1000, alpha=.5, beta=.15, gamma=.05, w1=10.0, w2=3.0, shift=0.0,
        # validation
        n_images=5,
        # build-side: the step's three Adams as one HIP launch (optim.FusedAdam / FusedAdamSet)
        dg_fused_adam=False,
        # build-side: the featurizer is featurizer.DinoFeaturizer (the ViT of vit.py) instead of StandInFeaturizer; its attention
        # through the fused HIP kernel (ops.attention_forward), its blocks' linear layers through ops.vit_linear_forward
        # (dg_dino_vit_kwargs: test hook, constructor arguments of the ViT that override the architecture's)
        dg_dino_backbone=False, dg_fused_attention=False, dg_fused_linear=False, dg_dino_vit_kwargs=None,
        # arch "dino_depth" (above: "dino"): how DinoFeaturizerWithDepth mixes the depth encoder's map into the features -
        # "sum", "cross_attn", "concat" or "none" (src/modules.py:526-528)
        guidance="none",
        # build-side, arch "dino_depth" with n_feats == 384: the depth encoder as one fused HIP forward and backward (depth_encoder.py)
        dg_fused_depth_encoder=False,
        # build-side, the same arch under guidance "cross_attn": the attention core between cross_attn's projections as one fused HIP
        # forward and backward (cross_attn.py)
        dg_fused_cross_attn=False,
        # the same arch under guidance "sum" / "cross_attn" with rec_weight > 0 (refused without this key): the reconstruction term
        # reads the featurizer's ATTACHED feats and its backward writes d feats as well (rec_loss.reconstruction_loss(feats_grad=True)),
        # so the term trains the depth modules as in the reference; under any other arch or guidance the key changes nothing
        dg_rec_feats_grad=False,
        # build-side, arch "dino": None, or the storage type ("float32", "float16", "bfloat16") of a feature_cache.FeatureCache - a
        # batch that carries `image_feat` / `image_feat_pos` (data.ContrastiveBatches(feature_cache=...)) then skips the frozen backbone
        dg_feature_cache=None,
        # build-side, arch "dino": None, or the storage type of a FeatureCache of the VAL split (train.val_feature_cache) - a val batch
        # that carries `image_feat` (data.ContrastiveBatches(pos=False, feature_cache=...)) then skips the frozen backbone in
        # validation_step and evaluate_batch
        dg_val_feature_cache=None,
        # build-side: the cached step recorded in a hipGraph and replayed, its batches drawn on the device (graph_step.GraphedTrainStep
        # over epoch.DeviceEpoch; the train command's --graph-step).  training_step itself does not read the key
        dg_graph_step=False,
        # build-side: both probes of the step and their parameter gradients as one fused HIP operation on the detached code
        # (head.fused_probe_losses; the train command's --fused-probes).  Read once, when the segmenter is constructed
        dg_fused_probes=False,
        # depth_sampling "fps_depth_feat" only: True draws the sample grid with the feature-aware sampler (ops.fps_feats_coords_pair, the
        # reference's uncalled fps_depth_feats); False keeps the reference's behaviour, where that mode is 'fps' (quirk Q13)
        dg_fps_feats=False)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg
