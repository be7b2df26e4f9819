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

`segment` is the label-free route (src/demo_segmentation.py:59-78): the same projection and resize, then the cluster ids' remap
through the Hungarian assignment, byte label maps of every image and, on request, painted images - one HIP launch pair
(ops.segment_labels -> dg_segment_labels, depthg_amd/csrc/dg_seg_labels.hip), or the CRF's predictions through ops.label_paint.
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


class Segmentation:
    """What `segment` returns: `.linear` / `.cluster` uint8 (B,H,W) label maps (255: no class), `.linear_rgb` / `.cluster_rgb` uint8
    (B,H,W,3) painted images, or None when no overlay was asked for."""
    __slots__ = ("linear", "cluster", "linear_rgb", "cluster_rgb")

    def __init__(self, linear, cluster, linear_rgb=None, cluster_rgb=None):
        self.linear, self.cluster, self.linear_rgb, self.cluster_rgb = linear, cluster, linear_rgb, cluster_rgb


def cluster_remap(cluster_metrics, m):
    """The (m,) int64 table cluster id -> class id of a metric whose `compute()` has formed `assignments` (the Hungarian matching,
    UnsupervisedMetrics.map_clusters; -1: an unmatched extra cluster), or None when it has none."""
    if cluster_metrics is None or getattr(cluster_metrics, "assignments", None) is None:
        return None
    table = torch.as_tensor(cluster_metrics.map_clusters(torch.arange(m))).reshape(-1).to(torch.int64)
    if table.numel() != m:
        raise ValueError(f"depthg_amd: the metric's assignment maps {table.numel()} clusters, the cluster probe has {m}")
    return table


def _segment_torch(code, size, lin_w, lin_b, clusters, code_flip, remap, img, alpha):
    """The reference's chain in plain torch (src/demo_segmentation.py:59-78 without the CRF), for tensors on the CPU."""
    import torch.nn.functional as F
    n, m = lin_w.shape[0], clusters.shape[0]
    if n > 255 or m > 255:
        raise ValueError(f"depthg_amd: a byte label map holds at most 255 classes and clusters (got {n}, {m})")
    code = code.float()
    if code_flip is not None:
        code = (code + code_flip.float().flip(dims=[3])) / 2
    up = F.interpolate(code, tuple(size), mode="bilinear", align_corners=False)
    lin = F.conv2d(up, lin_w.float().reshape(n, -1, 1, 1), None if lin_b is None else lin_b.float()).argmax(1)
    clu = torch.einsum("bchw,nc->bnhw", F.normalize(up, dim=1), F.normalize(clusters.float(), dim=1)).argmax(1)
    if remap is not None:
        clu = remap.to(torch.int64)[clu]
        clu = torch.where((clu < 0) | (clu > 254), torch.full_like(clu, 255), clu)
    lin, clu = lin.to(torch.uint8), clu.to(torch.uint8)
    if alpha is None:
        return Segmentation(lin, clu)
    a = int(round(float(alpha) * 256))
    cmap = ops.pascal_colormap().to(torch.int64)
    pix = 0
    if a < 256:
        mean, std = (torch.tensor(v, dtype=torch.float32).reshape(1, 3, 1, 1) for v in (ops.IMAGENET_MEAN, ops.IMAGENET_STD))
        pix = ((img.float() * std + mean) * 255).round().clamp(0, 255).to(torch.int64).permute(0, 2, 3, 1)
    paint = lambda lab: ((a * cmap[lab.to(torch.int64)] + (256 - a) * pix + 128) >> 8).to(torch.uint8)      # noqa: E731
    return Segmentation(lin, clu, paint(lin), paint(clu))


def segment(code: torch.Tensor, size, linear_probe, cluster_probe, code_flip: Optional[torch.Tensor] = None, cluster_metrics=None,
            run_crf: bool = False, img: Optional[torch.Tensor] = None, overlay: Optional[float] = None) -> Segmentation:
    """Label-free inference (src/demo_segmentation.py:59-78): the label maps of `linear_probe` and `cluster_probe` on `code`
    (B,dim,h,w) resized to `size` = (H, W), for every image, as bytes - no label, no metric.  `code_flip`: the code of the mirrored
    images, averaged in as at evaluation.  `cluster_metrics`: an UnsupervisedMetrics whose compute() has run - its Hungarian
    assignment turns the cluster ids into class ids (unmatched: 255); without it the raw cluster ids are stored, as the reference
    demo does.  `overlay`: None, or the weight in [0, 1] of the PASCAL colours over the de-normalised `img` (B,3,H,W) in the two
    painted images (1: the colours alone, `img` not needed).  `run_crf`: refine both probes with the dense CRF first (needs `img`).
    On the GPU one fused HIP launch pair (ops.segment_labels), or ops.segment_unary -> ops.dense_crf -> ops.label_paint with
    run_crf; tensors on the CPU take the reference's torch chain, which has no CRF."""
    H, W = (int(v) for v in size)
    lin_w, lin_b, clusters = linear_probe.weight, linear_probe.bias, cluster_probe.clusters
    m = clusters.shape[0]
    remap = cluster_remap(cluster_metrics, m)
    if overlay is not None and not 0.0 <= float(overlay) <= 1.0:
        raise ValueError(f"depthg_amd: overlay must lie in [0, 1], got {overlay}")
    blend = overlay is not None and int(round(float(overlay) * 256)) < 256
    if (run_crf or blend) and img is None:
        raise ValueError("depthg_amd: run_crf and an overlay below 1 need the images (img)")
    if img is not None and (img.dim() != 4 or tuple(img.shape) != (code.shape[0], 3, H, W)):
        raise ValueError(f"depthg_amd: img must be (B={code.shape[0]}, 3, {H}, {W}), the size asked for, got {tuple(img.shape)}")
    want = ("lin", "clu") + (("lin_rgb", "clu_rgb") if overlay is not None else ())
    alpha = 1.0 if overlay is None else float(overlay)
    with torch.no_grad():
        if not code.is_cuda:
            if run_crf:
                raise RuntimeError("depthg_amd: the dense CRF runs on the GPU only (dg_dense_crf); move the tensors and the probes to "
                                   "the GPU, or call segment with run_crf=False")
            lin_w = lin_w.reshape(lin_w.shape[0], -1)
            return _segment_torch(code, (H, W), lin_w, lin_b, clusters, code_flip, remap, img, overlay)
        if run_crf:
            n = lin_w.shape[0]
            U = ops.segment_unary(code, lin_w, lin_b, clusters, H, W, code_flip=code_flip, alpha=2.0)
            _, preds = ops.dense_crf(img, U, [n, n + m], n_iter=crf.MAX_ITER, pos_w=crf.POS_W, pos_xy_std=crf.POS_XY_STD, bi_w=crf.Bi_W,
                                     bi_xy_std=crf.Bi_XY_STD, bi_rgb_std=crf.Bi_RGB_STD, return_q=False, return_preds=True)
            out = ops.label_paint(preds, m=m, remap=remap, img=img, alpha=alpha, want=want)
        else:
            out = ops.segment_labels(code, lin_w, lin_b, clusters, H, W, code_flip=code_flip, remap=remap, img=img, alpha=alpha, want=want)
    return Segmentation(out["lin"], out["clu"], out.get("lin_rgb"), out.get("clu_rgb"))


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
