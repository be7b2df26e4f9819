"""Host mirror of the caller arithmetic around the correlation loss:
`LitUnsupervisedSegmenter.training_step`, reference src/train_segmentation.py:240-350 - the means of the returned
tuple, the log keys, and the weighted correspondence total including the `correspondence_weight - balance` factor
and the optional second (LHP) evaluation of the loss.  Pure host/torch-scalar logic on the tuple the module returns;
nothing here touches the HIP library, so it runs on any device the tuple lives on.

    out = loss_fn(feats, feats_pos, sal, sal_pos, code, code_pos, depth, depth_pos)
    total, logs = correspondence_total(cfg, out)                 # what `loss += ...` adds at :335-350
    total.backward()

`step_plan(cfg, ...)` is the host-side plan of one UnsupervisedSegmenter.training_step - every switch the step reads, decided once;
`histogram_step` / `reset_probe_step` are its two step-number predicates, shared with graph_step.GraphedTrainStep.
`fused_correspondence_total(cfg, loss_fn)` is the same number as formed inside the library (`loss_fn.total`, no torch op at
all; what bench.py times).
"""
from collections import namedtuple
from typing import Dict, Optional, Sequence, Tuple

import torch

LOG_KEYS_LOSS = ("loss/pos_intra", "loss/pos_inter", "loss/neg_inter", "loss/depth_feat")
LOG_KEYS_CD = ("cd/pos_intra", "cd/pos_inter", "cd/neg_inter", "cd/depth_feat")


def histogram_step(cfg, global_step: int) -> bool:
    """Whether step `global_step` histograms the cd tensors (src/train_segmentation.py:229-231, 298-301: inside the correspondence
    branch, every cfg.hist_freq steps, never at step 0): one more launch, three more logs."""
    hist_freq = getattr(cfg, "hist_freq", None)
    return cfg.correspondence_weight > 0 and hist_freq is not None and global_step % hist_freq == 0 and global_step > 0


def reset_probe_step(cfg, global_step: int) -> bool:
    """Whether step `global_step` ends by resetting the probes and their optimisers (src/train_segmentation.py:451-455)."""
    return cfg.reset_probe_steps is not None and global_step == cfg.reset_probe_steps


# Every switch UnsupervisedSegmenter.training_step reads.  route: the featurizer passes - "pair" (both at once), "depth" ((img, depth),
# one at a time) or "single"; cached: they start from batch["image_feat"] / ["image_feat_pos"], behind the backbone; correspondence,
# rec, aug, crf: the term's weight is > 0; depth_term, use_salience: cfg's, under correspondence; histograms, reset_probes: the two
# predicates above for this step; gpu_augment: None (off), "unit" (colour ops on de-normalised values) or "given" (any other true value).
StepPlan = namedtuple("StepPlan", "route cached correspondence lhp depth_term use_salience depth_only_intra histograms hist_bins "
                                  "rec aug crf rec_feats_grad gpu_augment fused_adam reset_probes")


def step_plan(cfg, *, net, batch, depth_arch: bool, depth_only_intra: bool, global_step: int) -> StepPlan:
    """The plan of one training step: cfg read once, each absent key's default stated here and nowhere else in the step (the keys the
    reference always has - correspondence_weight, use_salience, depth_feat_correlation_loss, reset_probe_steps - are attributes, read
    where the step needs them, as before).  Host logic: no tensor is touched beyond `key in batch`.  Reading the switches in front of
    the step changes nothing: inside a step cfg is written by legacy_decay_step (depth_feat_weight, depth_feat_shift, depth_sampling,
    feature_samples) and correspondence_total (lhp_weight) only - no switch of the plan.  The loss's weights are read where they are used."""
    correspondence = cfg.correspondence_weight > 0
    lhp = bool(getattr(cfg, "lhp", False))
    # both passes at once where nothing that draws random numbers stands between them in the reference - the LHP module does - and
    # the featurizer offers it; the depth-guided featurizer takes (img, depth) and returns four values, :191-200, one pass at a time
    paired = correspondence and not lhp and hasattr(net, "forward_pair") and net.training and not depth_arch
    cached = bool(getattr(cfg, "dg_feature_cache", None)) and "image_feat" in batch and "image_feat_pos" in batch and \
        not depth_arch and hasattr(net, "forward_pair_features")
    gpu_augment = getattr(cfg, "dg_gpu_augment", False)
    return StepPlan(route="pair" if paired else "depth" if depth_arch else "single", cached=cached, correspondence=correspondence, lhp=lhp,
                    depth_term=correspondence and bool(cfg.depth_feat_correlation_loss),
                    use_salience=correspondence and bool(cfg.use_salience), depth_only_intra=bool(depth_only_intra),
                    histograms=histogram_step(cfg, global_step), hist_bins=int(getattr(cfg, "dg_hist_bins", 64)),
                    rec=getattr(cfg, "rec_weight", 0) > 0, aug=getattr(cfg, "aug_alignment_weight", 0) > 0,
                    crf=getattr(cfg, "crf_weight", 0) > 0, rec_feats_grad=bool(getattr(cfg, "dg_rec_feats_grad", False)),
                    gpu_augment=("unit" if gpu_augment == "unit" else "given") if gpu_augment else None,
                    fused_adam=bool(getattr(cfg, "dg_fused_adam", False)), reset_probes=reset_probe_step(cfg, global_step))


def _balance(cfg) -> float:
    # src/train_segmentation.py:325-328: only the depth branch subtracts the LHP weight
    return float(cfg.lhp_weight) if getattr(cfg, "lhp", False) and getattr(cfg, "lhp_weight_balance", False) else 0.0


def correspondence_total(cfg, out: Sequence[torch.Tensor], lhp_out: Optional[Sequence[torch.Tensor]] = None
                         ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """`out`: the 6- or 8-tuple of ContrastiveCorrelationLoss (8 iff cfg.depth_feat_correlation_loss);
    `lhp_out`: the tuple of the second call on the LHP-projected code when cfg.lhp (src/train_segmentation.py:255-266,
    281-292), else None.  Returns (term added to the training loss, {log key: detached scalar})."""
    depth = len(out) == 8
    if depth != bool(getattr(cfg, "depth_feat_correlation_loss", False)):
        raise ValueError(f"tuple of {len(out)} does not match cfg.depth_feat_correlation_loss")
    pos_intra, pos_inter, neg_inter = out[0].mean(), out[2].mean(), out[4].mean()        # :303-305
    logs = {"loss/pos_intra": pos_intra.detach(), "loss/pos_inter": pos_inter.detach(), "loss/neg_inter": neg_inter.detach(),
            "cd/pos_intra": out[1].mean().detach(), "cd/pos_inter": out[3].mean().detach(), "cd/neg_inter": out[5].mean().detach()}
    core = cfg.pos_inter_weight * pos_inter + cfg.pos_intra_weight * pos_intra + cfg.neg_inter_weight * neg_inter
    if depth:
        depth_feat = out[6].mean()                                                        # :312-316
        logs["loss/depth_feat"] = depth_feat.detach()
        logs["cd/depth_feat"] = out[7].mean().detach()
        total = (core + cfg.depth_feat_weight * depth_feat) * (cfg.correspondence_weight - _balance(cfg))   # :330-333
        if "lhp_original" in str(getattr(cfg, "experiment_name", "")):                    # :335-337: only the LHP terms train,
            total = torch.zeros((), dtype=total.dtype, device=total.device)              # `loss = 0.0` (:336): a nan/inf main term
                                                                                          # is dropped, not turned into 0 * inf
            cfg.lhp_weight = 1.0
    else:
        total = core * cfg.correspondence_weight                                          # :347-349
    if getattr(cfg, "lhp", False) and depth:                                              # :339-343 (depth branch only)
        if lhp_out is None:
            raise ValueError("cfg.lhp is set: pass the tuple of the second loss call on the projected code")
        lhp_depth = lhp_out[6].mean() if len(lhp_out) == 8 else 0.0
        total = total + (cfg.pos_inter_weight * lhp_out[2].mean() + cfg.pos_intra_weight * lhp_out[0].mean() +
                         cfg.neg_inter_weight * lhp_out[4].mean() +
                         cfg.depth_feat_weight * cfg.lhp_depth_weight * lhp_depth) * cfg.lhp_weight
    return total, logs


def correspondence_weights(cfg, depth: bool, device, full: bool = False) -> torch.Tensor:
    """fp32 [4] weights of (intra, inter, neg, depth) loss means in the total, in the order of the fused output vector;
    `full`: zero-padded to the length of the fused output vector, so that `dot(loss_fn.scalars, w)` needs no slice (and its backward
    no zero-fill + copy)."""
    scale = (cfg.correspondence_weight - _balance(cfg)) if depth else cfg.correspondence_weight
    w = torch.tensor([cfg.pos_intra_weight, cfg.pos_inter_weight, cfg.neg_inter_weight,
                      cfg.depth_feat_weight if depth else 0.0] + ([0.0] * 5 if full else []), dtype=torch.float32)
    return (w * scale).to(device)


def fused_correspondence_total(cfg, loss_fn) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """Same value as correspondence_total(cfg, out) for the last call of `loss_fn` (without LHP): the library's own
    weighted total."""
    s = loss_fn.scalars
    depth = bool(getattr(cfg, "depth_feat_correlation_loss", False))
    total = loss_fn.total                      # formed by the library with the weights of cfg (DG_OUT_TOTAL)
    d = s.detach()
    logs = {k: d[i] for i, k in enumerate(LOG_KEYS_LOSS[:4 if depth else 3])}
    logs.update({k: d[4 + i] for i, k in enumerate(LOG_KEYS_CD[:4 if depth else 3])})
    return total, logs
