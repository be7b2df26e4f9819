"""The dense CRF on images with flat colour regions (flat_region_images of test_crf_cpu.py) against the numpy restatement of
tests/crf_reference.py.

On the noise images of test_gpu_crf.py no splat run is longer than 4 entries, so a run crosses one CRF_TILE boundary at the most.
Here hundreds to thousands of pixels share a bilateral vertex and a run crosses many: whole tiles of one vertex in
k_crf_splat_tail, several partial sums read back in tile order by k_crf_splat_head and the per-image cut of the tiles under a long
run carry the result, and the build kernels sort, mark and scan long rows of equal keys, clamp
colours at exactly 0 and 255 and elevate features that lie on lattice planes (test_crf_cpu.py asserts the run lengths of these very
images).  Bounds as in test_gpu_crf.py: filter relative error <= 1e-5, asymmetry within 2e-6 of the restatement's, mean field
max|dQ| <= 1e-4 at 37 x 53; at 96 x 128 the bound comes from the restatement's own sensitivity (see the test)."""
import functools

import numpy as np
import pytest
import torch

import crf_reference as R
from test_crf_cpu import FLAT_SEED, flat_region_images
from test_gpu_crf import DEV, _dense_case, _eval_case, check_preds, check_run_crf_chain

pytestmark = pytest.mark.gpu
SHAPES = [(37, 53), (96, 128)]


def flat_images(B, H, W, single_colour=False):
    return flat_region_images(np.random.default_rng(FLAT_SEED), B, H, W, single_colour=single_colour)


@functools.lru_cache(maxsize=None)
def lattices(H, W, B, single_colour=False):
    """The restatement's lattices of flat_images(B, H, W) with their norms, built once: [(lattice, norm)] per image, and the
    Gaussian pair."""
    img = flat_images(B, H, W, single_colour)
    bil = [R.bilateral_lattice(img[b].numpy()) for b in range(B)]
    gau = R.gaussian_lattice(H, W)
    return [(lat, lat.norm()) for lat in bil], (gau, gau.norm())


def rows(x):
    """(C,H,W) -> the restatement's (H*W, C)"""
    return x.reshape(x.shape[0], -1).T


def check_filter(vals, img, H, W, single_colour=False):
    """ops.crf_filter of vals (B,C,H,W) on both kernels against the restatement's message: relative error <= 1e-5 per image."""
    from depthg_amd import ops
    B, C = vals.shape[:2]
    bil, gau = lattices(H, W, B, single_colour)
    out = {}
    for bilateral in (True, False):
        got = ops.crf_filter(torch.from_numpy(vals).to(DEV), img.to(DEV), bilateral=bilateral, sxy=67.0 if bilateral else 1.0,
                             srgb=3.0).cpu().numpy()
        for b in range(B):
            lat, nrm = bil[b] if bilateral else gau
            want = lat.message(rows(vals[b]), nrm).T.reshape(C, H, W)
            rel = np.abs(got[b] - want).max() / np.abs(want).max()
            print(f"flat filter {H} x {W} {'bilateral' if bilateral else 'Gaussian'} image {b}: relative error {rel:.2e}")
            assert rel <= 1e-5, (bilateral, b, rel)
        out[bilateral] = got
    return out


@pytest.mark.parametrize("field", ["values", "one_hot", "single_colour"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_crf_filter_on_flat_images_matches_restatement(shape, field):
    """B = 2, C = 6 through both kernels: random values, one-hot fields (the Q of confident pixels) and random values on images of
    a single colour, where every entry of an image falls on one of a dozen vertices."""
    H, W = shape
    B, C = 2, 6
    rng = np.random.default_rng(50)
    img = flat_images(B, H, W, field == "single_colour")
    if field == "one_hot":
        vals = np.ascontiguousarray(np.eye(C, dtype=np.float32)[rng.integers(0, C, (B, H, W))].transpose(0, 3, 1, 2))
    else:
        vals = rng.random((B, C, H, W)).astype(np.float32)
    check_filter(vals, img, H, W, field == "single_colour")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_indicator_of_a_flat_rectangle_and_its_complement_sum_to_the_constant_field(shape):
    """The indicator of the white rectangle puts whole tiles of weight on a few vertices and nothing elsewhere: a partial sum that
    is dropped or added twice moves its message by a tile's weight.  Each of the three messages (one call each) matches the
    restatement, and indicator + complement is the constant field's message to 1e-5 of its maximum."""
    H, W = shape
    img = flat_images(2, H, W)
    white = np.stack([(R.colour_image(img[b].numpy()) == 255).all(2) for b in range(2)])
    assert white.reshape(2, -1).sum(1).min() >= H * W // 5
    ind = white[:, None].astype(np.float32)
    msgs = [check_filter(f, img, H, W) for f in (ind, 1 - ind, np.ones_like(ind))]
    for bilateral in (True, False):
        a, b, one = (m[bilateral] for m in msgs)
        rel = np.abs(a + b - one).max() / np.abs(one).max()
        print(f"indicator + complement - constant, {H} x {W} {'bilateral' if bilateral else 'Gaussian'}: {rel:.2e}")
        assert rel <= 1e-5, (bilateral, rel)


def test_crf_filter_symmetry_on_a_flat_image_matches_the_restatement():
    """test_crf_filter_symmetry_matches_the_restatement on a flat-region image: <u, K~v> - <K~u, v> within 2e-6 of |u| |K~v| of the
    restatement's."""
    from depthg_amd import ops
    rng = np.random.default_rng(52)
    H, W = 37, 53
    img = flat_images(2, H, W)[:1]
    bil, gau = lattices(H, W, 2)
    u, v = (rng.random((1, 3, H, W)).astype(np.float32) for _ in range(2))
    for b in (False, True):
        kw = dict(bilateral=b, sxy=67.0 if b else 1.0, srgb=3.0)
        Kv = ops.crf_filter(torch.from_numpy(v).to(DEV), img.to(DEV), **kw).cpu().double().numpy()
        Ku = ops.crf_filter(torch.from_numpy(u).to(DEV), img.to(DEV), **kw).cpu().double().numpy()
        scale = np.linalg.norm(u) * np.linalg.norm(Kv)
        asym = ((u * Kv).sum() - (Ku * v).sum()) / scale
        lat, nrm = bil[0] if b else gau
        uf, vf = rows(u[0]), rows(v[0])
        asym_ref = (float((uf.astype(np.float64) * lat.message(vf, nrm)).sum())
                    - float((lat.message(uf, nrm).astype(np.float64) * vf).sum())) / scale
        print(f"flat symmetry {'bilateral' if b else 'Gaussian'}: asymmetry {asym:.3e}, restatement {asym_ref:.3e}")
        assert abs(asym_ref) > 1e-5 and abs(asym - asym_ref) <= 2e-6, (asym, asym_ref)


def test_dense_crf_on_flat_images_chunks_and_repeats_to_the_same_bits():
    """The per-image cut of the splat tiles: 6 * 37 * 53 entries per image are no multiple of CRF_TILE and the middle image's last
    sorted run is hundreds of entries long (test_crf_cpu.py), so in the batch of three it ends in a tile that is cut short.  A
    workspace of one image gives the bits of the whole batch at once, and two identical calls give the same bits."""
    from depthg_amd import _lib, ops
    ends, (H, W) = [3, 7], (37, 53)
    img, U, _ = _dense_case(np.random.default_rng(53), 3, ends, H, W, 10, 14, images=lambda rng, B, H, W: flat_images(B, H, W))
    one = _lib.load().dg_crf_workspace_bytes(1, H, W, 8, 3)
    assert 0 < one and _lib.load().dg_crf_workspace_bytes(2, H, W, 8, 3) > one
    q_all, p_all = ops.dense_crf(img.to(DEV), U, ends, return_preds=True)
    q_again, p_again = ops.dense_crf(img.to(DEV), U, ends, return_preds=True)
    q_one, p_one = ops.dense_crf(img.to(DEV), U, ends, return_preds=True, workspace_budget=one)
    assert torch.equal(q_all, q_again) and torch.equal(p_all, p_again)
    assert torch.equal(q_all, q_one) and torch.equal(p_all, p_one)


def restatement_sensitivity(img, U, ends):
    """How far the restatement's own Q moves under roundings the GPU is free to make differently: (max|Q32 - Q64|, the fp32 chain
    against the same lattices accumulated in float64; max|Q32(U) - Q32(U')|, U' = U moved by 1 ulp up or down per element),
    and Q32."""
    q32 = R.dense_crf(img, U, ends)
    q64 = R.dense_crf(img, U, ends, dtype=np.float64)
    up = np.random.default_rng(7).integers(0, 2, U.shape).astype(bool)
    U1 = np.where(up, np.nextafter(U, np.float32(np.inf)), np.nextafter(U, np.float32(-np.inf))).astype(np.float32)
    return float(np.abs(q32 - q64).max()), float(np.abs(q32 - R.dense_crf(img, U1, ends)).max()), q32


MEAN_FIELD_CASES = {(37, 53): (2, 55), (96, 128): (1, 54)}       # shape: (B, the seed of the logits)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_crf_on_flat_images_matches_restatement(shape):
    """Mean field with groups [3, 7] on flat-region images, ten iterations, the GPU and the restatement on the same bits of U
    (the restatement's; the GPU's unary is held to its own bound).  Ten iterations amplify rounding near decision boundaries, and
    on a flat region hundreds of pixels move together, so each bound is set against how far the restatement's own Q moves on the
    very input (restatement_sensitivity: its fp32 chain against float64 accumulation, and under 1 ulp of U), measured on the CPU:

    37 x 53 (B = 2): max|dQ| <= 1e-4, the bound of test_dense_crf_matches_restatement.  The restatement moves by 1.6e-6 / 5.1e-7
    (fp32 against float64, images 0 / 1) and 4.5e-6 / 2.3e-6 (1 ulp of U): 4 x the larger is 1.8e-5, within the bound, and the test
    asserts that before it looks at the GPU.  That is a condition on the input: with the logits of seed 54 the restatement's
    image 1 moves by 3.0e-5 and 3.6e-5 (4 x: 1.4e-4, and by 1.4e-4 under 3 ulp of U, the distance of the GPU's unary), so 1e-4
    cannot be asked of anyone there; seeds 55 .. 63 all meet the condition.

    96 x 128 (B = 1): the restatement moves by 9.15e-6 (fp32 against float64) and 4.44e-5 (1 ulp of U), so the bound is
    4 x 4.44e-5 = 1.78e-4 on every pixel (the GPU's order of summation is a third, independent rounding of the same chain), computed
    by the test from the restatement and capped at 1e-3."""
    from depthg_amd import ops
    H, W = shape
    ends, (B, seed) = [3, 7], MEAN_FIELD_CASES[shape]
    img, _, U_ref = _dense_case(np.random.default_rng(seed), B, ends, H, W, H // 4 + 1, W // 4 + 1,
                                images=lambda rng, B, H, W: flat_images(B, H, W))
    q, preds = ops.dense_crf(img.to(DEV), torch.from_numpy(U_ref).to(DEV), ends, return_q=True, return_preds=True)
    q, preds = q.cpu().numpy(), preds.cpu()
    for b in range(B):
        d64, dulp, Q_ref = restatement_sensitivity(img[b].numpy(), U_ref[b], ends)
        if H == 37:
            bound = 1e-4
            assert 4 * max(d64, dulp) <= bound, (d64, dulp)
        else:
            bound = min(1e-3, 4 * max(d64, dulp))
        px = np.abs(q[b] - Q_ref).max(0)
        print(f"flat dense_crf {H} x {W} image {b}: restatement fp32 - fp64 {d64:.2e}, under 1 ulp of U {dulp:.2e}, bound {bound:.2e}, "
              f"max|dQ| = {px.max():.3e}")
        assert px.max() <= bound, (px.max(), bound)
        check_preds(preds[:, b], Q_ref, ends)


def test_predict_and_score_run_crf_on_flat_images_matches_reference_chain():
    """The evaluation chain of test_predict_and_score_run_crf_matches_reference_chain, at its shape, on flat-region images."""
    check_run_crf_chain(_eval_case(23, images=lambda rng, B, H, W: flat_images(B, H, W)), True)
