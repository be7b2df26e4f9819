"""Scoring a segmenter: the probes' predictions at label resolution and the confusion counts of the validation metrics
(src/train_segmentation.py:471-499 validation_step, src/eval_segmentation.py:146-170, with or without the CRF).

The reference upsamples the code to the label resolution, runs the linear probe and the cluster probe on it, takes two arg-maxes
and bincounts them.  Both arg-maxes commute with the bilinear resize, so `predict_and_score` projects the code at feature
resolution and resizes only the (n + m)-row score maps, per label pixel, inside one HIP launch that also counts
(ops.segment_predict -> dg_segment_predict, depthg_amd/csrc/dg_eval.hip).  Flip test-time augmentation
((code + code_flip.flip(3)) / 2) happens inside the projection.

With run_crf=True (eval_config.yml's run_crf, src/eval_segmentation.py:162-167) both probes' outputs are refined by the dense CRF
(depthg_amd/crf.py) before the arg-max: the unary of both probes is written straight from the code (ops.segment_unary ->
dg_segment_unary), one mean-field call refines both as two channel groups (ops.dense_crf), and the metrics count its predictions.
"""
from typing import Optional, Tuple

import torch

from . import crf, ops


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
                      n_store: int = 0, img: Optional[torch.Tensor] = None,
                      run_crf: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Arg-max predictions of `linear_probe` (Conv2d(dim, n_classes, 1)) and `cluster_probe` (ClusterLookup) on `code` (B,dim,h,w)
    resized to the label resolution (bilinear, align_corners=False), counted into `linear_metrics.stats` and
    `cluster_metrics.stats` (UnsupervisedMetrics) in place.  `code_flip`: the code of the horizontally mirrored images; the
    prediction is then made on (code + code_flip.flip(3)) / 2.  Returns (linear_preds, cluster_preds), int64 (n_store,H,W) of the
    first `n_store` images, or (None, None) when n_store is 0.
    run_crf: refine both probes' outputs (log_softmax of the linear probe, of the cluster probe with alpha = 2) with the dense CRF
    before the arg-max (src/eval_segmentation.py:162-167); needs `img` (B,3,H,W), the normalised images at the label size."""
    weight = linear_probe.weight
    n = weight.shape[0]
    for name, mt in (("linear_metrics", linear_metrics), ("cluster_metrics", cluster_metrics)):
        if mt is not None and mt.n_classes != n:
            raise ValueError(f"depthg_amd: {name} counts {mt.n_classes} classes, the linear probe predicts {n}")
    dev = code.device
    stats_lin = _metric_state(linear_metrics, dev)
    stats_clu = _metric_state(cluster_metrics, dev)
    if run_crf:
        return _predict_crf(code, label, weight, linear_probe.bias, cluster_probe.clusters, linear_metrics, cluster_metrics,
                            code_flip, n_store, img)
    with torch.no_grad():
        return ops.segment_predict(code, label, weight, linear_probe.bias, cluster_probe.clusters, code_flip=code_flip,
                                   stats_lin=stats_lin, stats_clu=stats_clu, n_store=n_store)


def _predict_crf(code, label, lin_w, lin_b, clusters, linear_metrics, cluster_metrics, code_flip, n_store, img):
    if img is None:
        raise ValueError("depthg_amd: run_crf needs the images (img)")
    H, W = label.shape[-2:]
    if img.dim() != 4 or tuple(img.shape[-2:]) != (H, W) or img.shape[0] != code.shape[0]:
        raise ValueError(f"depthg_amd: run_crf needs img (B={code.shape[0]}, 3, H, W) at the label size ({H}, {W}), got "
                         f"{tuple(img.shape)}")
    n_store = int(n_store)
    if n_store < 0:
        raise ValueError(f"depthg_amd: n_store must be >= 0, got {n_store}")
    n = lin_w.shape[0]
    with torch.no_grad():
        U = ops.segment_unary(code, lin_w, lin_b, clusters, H, W, code_flip=code_flip, alpha=2.0)
        _, preds = ops.dense_crf(img, U, [n, n + clusters.shape[0]], n_iter=crf.MAX_ITER, pos_w=crf.POS_W, pos_xy_std=crf.POS_XY_STD,
                                 bi_w=crf.Bi_W, bi_xy_std=crf.Bi_XY_STD, bi_rgb_std=crf.Bi_RGB_STD, return_q=False,
                                 return_preds=True)
        lab = label.reshape(preds.shape[1:])
        if linear_metrics is not None:
            linear_metrics.update(preds[0], lab)
        if cluster_metrics is not None:
            cluster_metrics.update(preds[1], lab)
    if n_store == 0:
        return None, None
    n_store = min(n_store, code.shape[0])
    return preds[0, :n_store], preds[1, :n_store]
