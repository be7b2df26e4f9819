"""A vectorised numpy restatement of the dense CRF the reference runs (src/crf.py: pydensecrf's DenseCRF2D, densecrf 2.x), written
from the published algorithm (Kraehenbuehl & Koltun 2011; the permutohedral lattice of Adams et al. 2010) for the tests: the colour
image, the unary, the two Potts kernels with symmetric normalisation and mean-field inference.  fp32 where densecrf computes in
fp32; the lattice is built with np.unique and searchsorted.  Imported by the tests the way conftest is."""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
MEAN = np.array([0.485, 0.456, 0.406], F32)
STD = np.array([0.229, 0.224, 0.225], F32)
MAX_ITER, POS_W, POS_XY_STD, BI_W, BI_XY_STD, BI_RGB_STD = 10, 3.0, 1.0, 4.0, 67.0, 3.0


def colour_image(img):
    """img (3,H,W) normalised fp32 -> uint8 (H,W,3) in BGR order: v = x * std + mean (two fp32 roundings), trunc(v * 255), clamped."""
    x = np.asarray(img, F32)
    v = x * STD[:, None, None]
    v = v + MEAN[:, None, None]
    t = np.clip(v * F32(255), F32(0), F32(255))
    t = np.where(np.isnan(t), F32(0), t)
    return np.ascontiguousarray(np.trunc(t).astype(np.uint8).transpose(1, 2, 0)[:, :, ::-1])


def features(H, W, sxy, bgr=None, srgb=None):
    """(H*W, d) fp32: (x, y) / sxy, then (B, G, R) / srgb when bgr (H,W,3) is given; x the column, y the row."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cols = [x.reshape(-1).astype(F32) / F32(sxy), y.reshape(-1).astype(F32) / F32(sxy)]
    if bgr is not None:
        for c in range(3):
            cols.append(bgr[:, :, c].reshape(-1).astype(F32) / F32(srgb))
    return np.stack(cols, 1)


class Lattice:
    """The permutohedral lattice of features (N, d): per pixel the d + 1 vertices (offsets) and barycentric weights, the blur
    neighbours of every vertex per direction (index M: the zero row)."""

    def __init__(self, feat):
        feat = np.asarray(feat, F32)
        N, d = feat.shape
        self.N, self.d = N, d
        scale = np.array([1.0 / np.sqrt((i + 2) * (i + 1)) * np.sqrt(2.0 / 3.0) * (d + 1) for i in range(d)]).astype(F32)
        cf = feat * scale
        el = np.zeros((N, d + 1), F32)
        sm = np.zeros(N, F32)
        for j in range(d, 0, -1):
            el[:, j] = sm - F32(j) * cf[:, j - 1]
            sm = sm + cf[:, j - 1]
        el[:, 0] = sm
        down, up = F32(1.0 / (d + 1)), F32(d + 1)
        v = down * el
        hi, lo = np.ceil(v) * up, np.floor(v) * up
        rem0 = np.where(hi - el < el - lo, hi, lo).astype(np.int64)
        s = rem0.sum(1) // (d + 1)
        dl = el - rem0.astype(F32)
        rank = np.zeros((N, d + 1), np.int64)
        for i in range(d):
            for j in range(i + 1, d + 1):
                c = dl[:, i] < dl[:, j]
                rank[:, i] += c
                rank[:, j] += ~c
        rank += s[:, None]
        neg, big = rank < 0, rank > d
        rank[neg] += d + 1
        rem0[neg] += d + 1
        rank[big] -= d + 1
        rem0[big] -= d + 1
        vv = (el - rem0.astype(F32)) * down
        vr = np.zeros((N, d + 1), F32)
        np.put_along_axis(vr, rank, vv, 1)
        bary = np.zeros((N, d + 1), F32)
        bary[:, 0] = (vr[:, d].astype(np.float64) + (1.0 - vr[:, 0].astype(np.float64))).astype(F32)
        for k in range(1, d + 1):
            bary[:, k] = vr[:, d - k] - vr[:, d - k + 1]
        keys = np.empty((N, d + 1, d), np.int64)
        for r in range(d + 1):
            keys[:, r, :] = rem0[:, :d] + np.where(rank[:, :d] <= d - r, r, r - (d + 1))
        flat = keys.reshape(-1, d)
        base = flat.min(0) - 2 * (d + 1)
        span = flat.max(0) - base + 2 * (d + 1) + 1
        mult = np.ones(d, np.int64)
        for i in range(d - 2, -1, -1):
            mult[i] = mult[i + 1] * span[i + 1]
        assert float(np.prod(span.astype(np.float64))) < 2.0 ** 62
        packed = ((flat - base) * mult).sum(1)
        uniq, inv = np.unique(packed, return_inverse=True)
        self.M = M = len(uniq)
        self.offsets = inv.reshape(N, d + 1)
        self.bary = bary
        self.nbrs = np.empty((d + 1, M, 2), np.int64)
        for j in range(d + 1):
            delta = np.full(d, -1, np.int64)
            if j < d:
                delta[j] = d
            step = (delta * mult).sum()
            for t, want in enumerate((uniq + step, uniq - step)):
                pos = np.minimum(np.searchsorted(uniq, want), M - 1)
                self.nbrs[j, :, t] = np.where(uniq[pos] == want, pos, M)
        order = np.argsort(self.offsets.reshape(-1), kind="stable")
        self._order = order
        self._starts = np.flatnonzero(np.r_[True, np.diff(self.offsets.reshape(-1)[order]) != 0])
        self.alpha = F32(1.0) / (F32(1.0) + F32(2.0) ** F32(-d))

    def filter(self, vals, dtype=F32):
        """K(vals) (N, C), without normalisation: splat, blur in directions 0..d, slice with alpha.  dtype: the type the three steps
        accumulate in (fp32 as densecrf; np.float64: the same vertices and fp32 weights, summed in double)."""
        vals = np.asarray(vals, dtype)
        d, M = self.d, self.M
        bary, half, alpha = self.bary.astype(dtype, copy=False), dtype(0.5), dtype(self.alpha)
        contrib = bary.reshape(-1)[self._order, None] * vals[self._order // (d + 1)]
        V = np.zeros((M + 1, vals.shape[1]), dtype)
        V[:M] = np.add.reduceat(contrib, self._starts, axis=0)
        for j in range(d + 1):
            W = np.zeros_like(V)
            W[:M] = V[:M] + half * (V[self.nbrs[j, :, 0]] + V[self.nbrs[j, :, 1]])
            V = W
        out = np.zeros_like(vals)
        for r in range(d + 1):
            out += (bary[:, r, None] * V[self.offsets[:, r]]) * alpha
        return out

    def norm(self, dtype=F32):
        k1 = self.filter(np.ones((self.N, 1), dtype), dtype)[:, 0]
        return (1.0 / np.sqrt(k1.astype(np.float64) + 1e-20)).astype(dtype)

    def message(self, vals, norm=None, dtype=F32):
        """The normalised message K~(vals) = norm * K(norm * vals) (NORMALIZE_SYMMETRIC), accumulated in dtype (see filter)."""
        norm = self.norm(dtype) if norm is None else norm
        return norm[:, None] * self.filter(norm[:, None] * np.asarray(vals, dtype), dtype)


def gaussian_lattice(H, W, sxy=POS_XY_STD):
    return Lattice(features(H, W, sxy))


def bilateral_lattice(img, sxy=BI_XY_STD, srgb=BI_RGB_STD):
    bgr = colour_image(img)
    return Lattice(features(bgr.shape[0], bgr.shape[1], sxy, bgr, srgb))


def softmax_groups(E, group_ends):
    """softmax over the channels of each group of E (N, C), the per-pixel maximum subtracted first."""
    out = np.empty_like(E)
    start = 0
    for end in group_ends:
        e = E[:, start:end]
        x = np.exp(e - e.max(1, keepdims=True))
        out[:, start:end] = x / x.sum(1, keepdims=True)
        start = end
    return out


def unary_from_logits(logits, H, W, group_ends=None):
    """U (C,H,W) fp32 of logits (C,h,w): torch's bilinear resize (align_corners=False) and softmax per group on the CPU, then
    -log(clip(p, 1e-5, 1)) (pydensecrf.utils.unary_from_softmax)."""
    lg = torch.as_tensor(np.asarray(logits, F32))
    up = F.interpolate(lg.unsqueeze(0), size=(H, W), mode="bilinear", align_corners=False)[0]
    ends = [lg.shape[0]] if group_ends is None else list(group_ends)
    probs, start = [], 0
    for end in ends:
        probs.append(F.softmax(up[start:end], dim=0))
        start = end
    p = torch.cat(probs).numpy()
    return -np.log(np.clip(p, F32(1e-5), F32(1.0)))


def dense_crf(img, U, group_ends=None, n_iter=MAX_ITER, pos_w=POS_W, pos_xy_std=POS_XY_STD, bi_w=BI_W, bi_xy_std=BI_XY_STD,
              bi_rgb_std=BI_RGB_STD, dtype=F32):
    """Mean field for one image: img (3,H,W) normalised, U (C,H,W).  Returns Q (C,H,W) in dtype (fp32 as densecrf; np.float64: the
    same lattices, with the messages and the softmax in double)."""
    C, H, W = U.shape
    ends = [C] if group_ends is None else list(group_ends)
    u = np.ascontiguousarray(np.asarray(U, F32).reshape(C, -1).T).astype(dtype, copy=False)
    Q = softmax_groups(-u, ends)
    if n_iter:
        lg, lb = gaussian_lattice(H, W, pos_xy_std), bilateral_lattice(img, bi_xy_std, bi_rgb_std)
        ng, nb = lg.norm(dtype), lb.norm(dtype)
        for _ in range(n_iter):
            E = -u + dtype(pos_w) * lg.message(Q, ng, dtype)
            E = E + dtype(bi_w) * lb.message(Q, nb, dtype)
            Q = softmax_groups(E, ends)
    return np.ascontiguousarray(Q.T.reshape(C, H, W))
