"""A numpy restatement of the reference's sample() (src/modules.py:822-825: F.grid_sample(t, coords.permute(0, 2, 1, 3),
padding_mode='border', align_corners=True), bilinear) as rows, for ops.sample_rows / dg_sample_rows.

The coordinate arithmetic - scale, clamp, floor, the four weights with the taps beyond the border zeroed - is float32 in the kernel's
order, so the taps and weights are the kernel's own; the blend of the four taps is float64.  Against it an fp32 row element may differ
by the blend's four roundings, each at most 2^-24 of a partial sum no larger than the largest tap (the weights are non-negative and
sum to 1 within their own roundings): SAMPLE_ROWS_ULPS = 8 of them covers those and, for a formulation that rounds the weight
products elsewhere, those too.  A bf16 element adds one bf16 rounding, 2^-8 of the value."""
import numpy as np

SAMPLE_ROWS_ULPS = 8

# (B, K, h, w): the smallest maps at which each part of the kernel can go wrong
SAMPLE_ROWS_SHAPES = [
    (2, 5, 3, 3),          # tiny map
    (2, 28, 136, 124),     # just above 16384 positions
    (1, 4, 256, 256),      # the limit
    (3, 6, 1, 300),        # one row: the y taps degenerate
    (2, 33, 130, 127),     # K not a multiple of 4, odd width
    (2, 130, 20, 20),      # a second pass of the lanes over the channels, and the bf16 pad to 256
]


def sample_map(seed, B, K, h, w):
    return np.random.default_rng(seed).standard_normal((B, K, h, w)).astype(np.float32)


def sample_coords(seed, B, S, Sh, h, w):
    """(B,S,Sh,2) float32 in [-1.3, 1.3]: beyond the border on every side; then, as far as the grid has room, exactly -1 and +1 and
    exact pixel centres."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.3, 1.3, (B, S, Sh, 2)).astype(np.float32)
    flat = c.reshape(-1, 2)
    fixed = [(-1.0, -1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -0.25)]
    for k in range(4):                                   # pixel centres: 2 i / (n - 1) - 1 (the centre itself where n = 1)
        ix, iy = int(rng.integers(0, w)), int(rng.integers(0, h))
        fixed.append((2.0 * ix / (w - 1) - 1.0 if w > 1 else 0.0, 2.0 * iy / (h - 1) - 1.0 if h > 1 else 0.0))
    step = max(1, flat.shape[0] // len(fixed))
    for k, xy in enumerate(fixed):
        if k * step < flat.shape[0]:
            flat[k * step] = xy
    return c


def sample_rows_reference(t, coords, srcidx=None):
    """t (B,K,h,w) float32, coords (B,S,Sh,2) -> (want, tapmax), both float64 (B, Sh*S, K): row p = i*S + j of image n is
    t[srcidx[n]] sampled at coords[n, j, i]; tapmax is the largest magnitude among the element's four taps."""
    t = np.asarray(t, dtype=np.float32)
    B, K, h, w = t.shape
    S, Sh = coords.shape[1], coords.shape[2]
    c = np.asarray(coords, dtype=np.float32).transpose(0, 2, 1, 3).reshape(B, Sh * S, 2)
    one, two, zero = np.float32(1), np.float32(2), np.float32(0)
    x = ((c[..., 0] + one) / two) * np.float32(w - 1)
    y = ((c[..., 1] + one) / two) * np.float32(h - 1)
    x = np.minimum(np.maximum(x, zero), np.float32(w - 1))
    y = np.minimum(np.maximum(y, zero), np.float32(h - 1))
    x0f, y0f = np.floor(x), np.floor(y)
    wx1, wy1 = x - x0f, y - y0f
    wx0, wy0 = one - wx1, one - wy1
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    inx, iny = x0 + 1 <= w - 1, y0 + 1 <= h - 1
    w00 = wy0 * wx0
    w01 = np.where(inx, wy0 * wx1, zero)
    w10 = np.where(iny, wy1 * wx0, zero)
    w11 = np.where(inx & iny, wy1 * wx1, zero)
    assert all(a.dtype == np.float32 for a in (x, wx0, w00, w01, w10, w11))
    pix, dx, dy = y0 * w + x0, inx.astype(np.int64), np.where(iny, w, 0)
    src = t if srcidx is None else t[np.asarray(srcidx)]
    flat = src.reshape(B, K, h * w).astype(np.float64)
    tap = lambda idx: np.take_along_axis(flat, idx[:, None, :], axis=2).transpose(0, 2, 1)          # (B, P, K)
    a00, a01, a10, a11 = tap(pix), tap(pix + dx), tap(pix + dy), tap(pix + dy + dx)
    W = lambda v: v.astype(np.float64)[..., None]
    want = a00 * W(w00) + a01 * W(w01) + a10 * W(w10) + a11 * W(w11)
    tapmax = np.maximum(np.maximum(np.abs(a00), np.abs(a01)), np.maximum(np.abs(a10), np.abs(a11)))
    return want, tapmax


def sample_rows_bound(want, tapmax, bf16):
    bound = SAMPLE_ROWS_ULPS * 2.0 ** -24 * tapmax
    return bound + 2.0 ** -8 * np.abs(want) if bf16 else bound


def check_rows(got, want, tapmax, K, bf16):
    """`got` (B,P,Kout) as float64 against the restatement, every element: -> the largest |got - want| / bound over the K channels
    (at most 1 when the rows pass); the padding K..Kout-1 must be exactly zero."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape[:2] == want.shape[:2] and got.shape[2] >= K
    assert np.isfinite(got).all(), "an element was not written (poison) or is not finite"
    assert not got[..., K:].any(), "the padding channels are not zero"
    bound = sample_rows_bound(want, tapmax, bf16)
    err = np.abs(got[..., :K] - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), f"max |got - want| / bound = {ratio:.3f}, max abs error {err.max():.3e}"
    return ratio
