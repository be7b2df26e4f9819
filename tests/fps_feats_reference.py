"""A plain numpy restatement of the feature-aware farthest point sampling (cfg.dg_fps_feats, ops.fps_feats_coords): the reference's
farthest_point_sampling_depth (src/modules.py:999-1037) with its `fps(point_cloud, n*n)` call replaced by
`fps_depth_feats(point_cloud, feats, n*n)` (:1124-1180) on the feature rows formed at :1017.  Restated without np.delete: a boolean
`left` mask plays the role of `points_left`, which stays in ascending order, so "first max over points_left" is "lowest index among
the maxima of the points not yet selected".  float32 as numpy runs the reference (its row sums included: `.sum(-1)` is numpy's own),
and a float64 variant that also reports every round's margin.  One deviation, the library's: where a round's maximum distance is 0
the reference divides 0 / 0 and selects on NaNs; here that term contributes 0.

Also the tests' inputs: `margin_inputs(seeds, ...)` draws a case from one seed per image, and CASES records the seeds tests/golden/fps_feats_*.npz
was generated with (scripts/make_fps_feats_fixtures.py searched them: a seed is accepted when every round's two largest running
distances differ by at least MARGIN of the larger in the float64 variant).  Imported by the tests the way conftest is."""
import numpy as np
import torch

from oracle import depthg_oracle as O

MARGIN = 1e-3        # (C + 2) * 2^-24 = 2.3e-5 at C = 384 bounds the direct fp32 distance's relative error: 40 times that

# name -> (one seed per image, C, h, w, H, W, S); the fixture of a case keeps its inputs when they are a few KB, its reference indices always
CASES = {
    "5x5": ((1,), 3, 5, 5, 5, 5, 2),
    "7x9": ((0,), 17, 7, 9, 21, 27, 3),
    "8x8_all": ((0,), 1, 8, 8, 16, 16, 8),
    "16x16": ((0,), 64, 16, 16, 32, 32, 5),
    "28x28": ((0, 30), 384, 28, 28, 56, 56, 11),
    "flat_depth": ((0,), 8, 6, 6, 12, 12, 3),
}


def margin_image(seed, C, h, w, H, W, S, flat_depth=False):
    """One image's depth (1,H,W) and feats (C,h,w), float32, from `seed` (numpy's RandomState: the stream is frozen).  S*S + 9 points
    (or all) at random places stand out: their depth and their feature amplitude are drawn log-uniformly over e^8, the others sit near
    depth 1 with features of amplitude 1e-3 - so the running distances of the points that compete for a round are far apart, which
    is what lets a seed hold the margin over all S*S rounds.  H, W multiples of h, w.  flat_depth: a constant map (a plane of points)."""
    rs = np.random.RandomState(seed)
    P, K = h * w, min(h * w, S * S + 9)
    out = rs.permutation(P)[:K]
    ad, af = np.full(P, 1.0), np.full(P, 1e-3)
    ad[out] = np.exp(rs.uniform(-4, 4, K))
    af[out] = np.exp(rs.uniform(-4, 4, K))
    depth = np.repeat(np.repeat(ad.reshape(h, w), H // h, 0), W // w, 1) * (1 + 1e-3 * rs.uniform(-1, 1, (H, W)))
    if flat_depth:
        depth = np.full((H, W), 2.0)
    feats = rs.standard_normal((C, h, w)) * af.reshape(1, h, w)
    return depth[None].astype(np.float32), feats.astype(np.float32)


def margin_inputs(seeds, C, h, w, H, W, S, flat_depth=False):
    """depth (B,1,H,W), feats (B,C,h,w): image b from seeds[b]."""
    both = [margin_image(s, C, h, w, H, W, S, flat_depth) for s in seeds]
    return np.stack([d for d, _ in both]), np.stack([f for _, f in both])


def points(depth, feat_hw):
    """depth (B,1,H,W) -> (B, h*w, 3) float32: adaptive_avg_pool2d to the feature grid, then depth2points(fov=90) (:1003, :1016)."""
    h, w = feat_hw
    d = O.adaptive_avg_pool2d(torch.as_tensor(np.asarray(depth, np.float32)), (h, w))
    return np.stack([O.depth2points(d[i, 0], fov=90.0).permute(1, 2, 0).reshape(-1, 3).numpy() for i in range(d.shape[0])])


def fps_depth_feats(pts, feats, n_samples, dtype=np.float32, want_margin=False):
    """pts (P,3), feats (P,C) -> the n_samples selected indices in selection order (and, want_margin, the smallest relative gap between
    a round's two largest running distances; rounds with one point left have none)."""
    pts, feats = np.asarray(pts, dtype), np.asarray(feats, dtype)
    n = pts.shape[0]
    left = np.ones(n, dtype=bool)
    dists = np.full(n, np.inf, dtype=np.float64)
    out = np.zeros(n_samples, dtype=np.int64)
    left[0] = False
    margin = np.inf
    for i in range(1, n_samples):
        last = out[i - 1]
        pd = ((pts[last] - pts) ** 2).sum(-1)
        fd = ((feats[last] - feats) ** 2).sum(-1)
        mp, mf = pd[left].max(), fd[left].max()
        tp = pd / mp if mp > 0 else np.zeros_like(pd)
        tf = fd / mf if mf > 0 else np.zeros_like(fd)
        d = np.sum((tp, tf), axis=0)
        dists = np.where(left, np.minimum(d, dists), dists)
        masked = np.where(left, dists, -np.inf)
        sel = int(np.argmax(masked))
        if want_margin and left.sum() > 1:
            top = np.sort(masked[left])[-2:]
            margin = min(margin, (top[1] - top[0]) / top[1] if top[1] > 0 else 0.0)
        out[i] = sel
        left[sel] = False
    return (out, margin) if want_margin else out


def sample(depth, feats, n_side, dtype=np.float32, want_margin=False):
    """depth (B,1,H,W), feats (B,C,h,w) -> coords (B,S,S,2) float32, already *2-1 (the selected set in row-major order, quirk Q4),
    and the selection order int64 (B, S*S); want_margin: also the smallest margin over the images."""
    feats = np.asarray(feats, np.float32)
    B, C, h, w = feats.shape
    pts = points(depth, (h, w))
    coords, inds, margin = [], [], np.inf
    for b in range(B):
        got = fps_depth_feats(pts[b], feats[b].transpose(1, 2, 0).reshape(-1, C), n_side * n_side, dtype, want_margin)
        if want_margin:
            got, m = got
            margin = min(margin, m)
        srt = np.sort(got)
        rows = (srt // w).astype(np.float32) / np.float32(h)
        cols = (srt % w).astype(np.float32) / np.float32(w)
        coords.append((np.stack([rows, cols], -1) * np.float32(2) - np.float32(1)).reshape(n_side, n_side, 2))
        inds.append(got)
    coords, inds = np.stack(coords).astype(np.float32), np.stack(inds)
    return (coords, inds, margin) if want_margin else (coords, inds)
