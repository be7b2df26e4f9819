"""Scoring a segmenter: the probes' predictions at label resolution and the confusion counts of the validation metrics
(src/train_segmentation.py:471-499 validation_step, src/eval_segmentation.py:146-170 without the CRF).

The reference upsamples the code to the label resolution, runs the linear probe and the cluster probe on it, takes two arg-maxes
and bincounts them.  Both arg-maxes commute with the bilinear resize, so `predict_and_score` projects the code at feature
resolution and resizes only the (n + m)-row score maps, per label pixel, inside one HIP launch that also counts
(ops.segment_predict -> dg_segment_predict, depthg_amd/csrc/dg_eval.hip).  Flip test-time augmentation
((code + code_flip.flip(3)) / 2) happens inside the projection.
"""
from typing import Optional, Tuple

import torch

from . import ops


def _metric_state(metrics, device):
    """The metric's `stats` on `device`, moved there the way UnsupervisedMetrics._accumulate moves it."""
    if metrics is None:
        return None
    state = metrics.stats
    if state.device != device:
        state = state.to(device)
        metrics.device = device
    if state.dtype != torch.int64 or not state.is_contiguous():
        raise ValueError("depthg_amd: the metric's stats must be a contiguous int64 matrix")
    metrics.stats = state
    return state


def predict_and_score(code: torch.Tensor, label: torch.Tensor, linear_probe, cluster_probe, linear_metrics=None,
                      cluster_metrics=None, code_flip: Optional[torch.Tensor] = None,
                      n_store: int = 0) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Arg-max predictions of `linear_probe` (Conv2d(dim, n_classes, 1)) and `cluster_probe` (ClusterLookup) on `code` (B,dim,h,w)
    resized to the label resolution (bilinear, align_corners=False), counted into `linear_metrics.stats` and
    `cluster_metrics.stats` (UnsupervisedMetrics) in place.  `code_flip`: the code of the horizontally mirrored images; the
    prediction is then made on (code + code_flip.flip(3)) / 2.  Returns (linear_preds, cluster_preds), int64 (n_store,H,W) of the
    first `n_store` images, or (None, None) when n_store is 0."""
    weight = linear_probe.weight
    n = weight.shape[0]
    for name, mt in (("linear_metrics", linear_metrics), ("cluster_metrics", cluster_metrics)):
        if mt is not None and mt.n_classes != n:
            raise ValueError(f"depthg_amd: {name} counts {mt.n_classes} classes, the linear probe predicts {n}")
    dev = code.device
    stats_lin = _metric_state(linear_metrics, dev)
    stats_clu = _metric_state(cluster_metrics, dev)
    with torch.no_grad():
        return ops.segment_predict(code, label, weight, linear_probe.bias, cluster_probe.clusters, code_flip=code_flip,
                                   stats_lin=stats_lin, stats_clu=stats_clu, n_store=n_store)
