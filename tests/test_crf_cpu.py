"""CPU-side checks of the dense CRF (dg_crf.hip, dg_crf_filter / dg_dense_crf / dg_crf_unary / dg_segment_unary, depthg_amd/crf.py,
predict_and_score(run_crf=True)): the exports, the refusals before any launch, the audit of dg_crf.hip's generated code and checks
of the numpy restatement the GPU tests compare against (tests/crf_reference.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import crf_reference as R

NEW = ["dg_crf_workspace_bytes", "dg_crf_unary", "dg_segment_unary", "dg_crf_filter", "dg_dense_crf"]


def normalised_images(rng, B, H, W):
    """T.Normalize of random uint8 images: many values sit within rounding of a truncation boundary of the colour chain."""
    u8 = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.float32) / 255)
    mean, std = torch.tensor([0.485, 0.456, 0.406])[:, None, None], torch.tensor([0.229, 0.224, 0.225])[:, None, None]
    return (u8 - mean) / std


def flat_region_images(rng, B, H, W, single_colour=False):
    """T.Normalize of uint8 images made of flat regions, the input that puts thousands of pixels on one bilateral vertex: over a
    horizontal ramp (green falling) a rectangle at exactly (255,255,255), one at exactly (0,0,0), one of a random colour and a
    patch of noise.  The white rectangle reaches the bottom right corner in images 0 and 1 (the largest features, so the last
    sorted run of the image is a long one); later images are mirrored (b % 3 == 2: left-right, b % 4 == 3: top-bottom), and
    the random colour and the noise differ in every image.  single_colour: every image is one random colour."""
    u8 = np.empty((B, 3, H, W), np.uint8)
    for b in range(B):
        if single_colour:
            u8[b] = rng.integers(0, 256, 3).astype(np.uint8)[:, None, None]
            continue
        ramp = np.round(np.arange(W) * (255.0 / max(W - 1, 1))).astype(np.uint8)
        im = np.broadcast_to(ramp, (3, H, W)).copy()
        im[1] = 255 - im[1]
        h2, w2, h3, w3 = H // 2, W // 2, H // 3, W // 3
        im[:, h2:, w2:] = 255
        im[:, :h3, :w2] = 0
        im[:, h3:h2, w3:2 * w3] = rng.integers(1, 255, 3).astype(np.uint8)[:, None, None]
        im[:, h2:h2 + h3 // 2 + 2, :w3] = rng.integers(0, 256, (3, h3 // 2 + 2, w3))
        if b % 3 == 2:
            im = im[:, :, ::-1]
        if b % 4 == 3:
            im = im[:, ::-1, :]
        u8[b] = im
    x = torch.from_numpy(u8.astype(np.float32) / 255)
    mean, std = torch.tensor([0.485, 0.456, 0.406])[:, None, None], torch.tensor([0.229, 0.224, 0.225])[:, None, None]
    return (x - mean) / std


FLAT_SHAPES = [(37, 53), (96, 128), (40, 48)]     # the shapes of the GPU tests on flat images (test_gpu_crf_flat.py)
FLAT_SEED = 40                            # those tests draw their images from this seed: the run lengths asserted here are theirs
CRF_TILE = 64                            # dg_crf.hip: a splat run is cut at every multiple of CRF_TILE sorted positions of its image


def test_crf_entry_points_are_declared_listed_and_exported():
    from depthg_amd import _lib
    import depthg_amd
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.dg_version() == 119
    for name in ("dense_crf", "batched_crf", "crf"):
        assert name in depthg_amd.__all__ and hasattr(depthg_amd, name)
    from depthg_amd import crf
    assert (crf.MAX_ITER, crf.POS_W, crf.POS_XY_STD, crf.Bi_W, crf.Bi_XY_STD, crf.Bi_RGB_STD) == (10, 3, 1, 4, 67, 3)
    # one image at 320 x 320 with 27 + 27 channels (56 padded) fits a 1 GiB budget twice
    one = lib.dg_crf_workspace_bytes(1, 320, 320, 56, 3)
    two = lib.dg_crf_workspace_bytes(2, 320, 320, 56, 3)
    assert 0 < one and 2 * one <= two + 4096 and two < 1 << 30
    assert lib.dg_crf_workspace_bytes(1, 320, 320, 54, 3) == 0       # Kp is a multiple of 4
    assert lib.dg_crf_workspace_bytes(1, 320, 320, 56, 0) == 0 and lib.dg_crf_workspace_bytes(1, 320, 320, 56, 4) == 0
    # a filter of one kernel carves only its own lattice
    g, b = lib.dg_crf_workspace_bytes(1, 320, 320, 56, 1), lib.dg_crf_workspace_bytes(1, 320, 320, 56, 2)
    assert 0 < g < b < one and g < one / 2


def test_chunks_whose_int_indices_would_overflow_are_refused():
    """The kernels index lattice entries x channel quads with int: (d + 1) c H W Kp / 4 must stay below 2^30."""
    from depthg_amd import _lib
    lib = _lib.load()
    assert lib.dg_crf_workspace_bytes(27, 320, 320, 256, 3) > 0          # 6 * 27 * 102400 * 64 < 2^30
    assert lib.dg_crf_workspace_bytes(28, 320, 320, 256, 3) == 0
    assert lib.dg_crf_workspace_bytes(54, 320, 320, 256, 1) > 0          # the Gaussian lattice alone: 3 entries per pixel
    assert lib.dg_crf_workspace_bytes(55, 320, 320, 256, 1) == 0
    assert lib.dg_crf_workspace_bytes(1, 4096, 4096, 256, 3) == 0        # one image near the pixel limit at 256 channels
    p = ctypes.c_void_p(256)
    ends = (ctypes.c_int32 * 1)(256)
    rc = lib.dg_dense_crf(p, p, 1, 4096, 4096, ends, 1, 10, 3.0, 1.0, 4.0, 67.0, 3.0, p, None, p, 1 << 40, None)
    assert rc == -2 and "2^30" in lib.dg_last_error().decode()


def _dense(ends=(3, 7), B=1, H=8, W=8, ws_bytes=1 << 40, ptr=256, n_iter=10, stds=(1.0, 67.0, 3.0)):
    from depthg_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(ptr)
    ce = (ctypes.c_int32 * max(1, len(ends)))(*ends)
    rc = lib.dg_dense_crf(p, p, B, H, W, ce, len(ends), n_iter, 3.0, stds[0], 4.0, stds[1], stds[2], p, None, p, ws_bytes, None)
    return rc, lib.dg_last_error().decode()


def test_dense_crf_refuses_bad_arguments_before_any_launch():
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(n_iter=-1)):
        rc, msg = _dense(**kw)
        assert rc == -1 and "dimensions" in msg, (kw, msg)
    for ends in ((), (0, 3), (3, 3), (4, 2), tuple(range(1, 10))):
        rc, msg = _dense(ends=ends)
        assert rc == -1 and "group ends" in msg, (ends, msg)
    rc, msg = _dense(stds=(0.0, 67.0, 3.0))
    assert rc == -1 and "positive" in msg
    rc, msg = _dense(ws_bytes=1000)
    assert rc == -3 and "workspace" in msg
    rc, msg = _dense(ptr=16)
    assert rc == -1 and "aligned" in msg
    # the packed keys of a 4096 x 4096 image at a bilateral position std of 0.001 need far more than 64 bits
    rc, msg = _dense(H=4096, W=4096, stds=(1.0, 1e-3, 3.0))
    assert rc == -2 and "63 bits" in msg
    rc, msg = _dense(H=4096, W=4096, stds=(1e-7, 67.0, 3.0))
    assert rc == -2 and "Gaussian" in msg


def test_filter_and_unary_refuse_bad_arguments_before_any_launch():
    from depthg_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    assert lib.dg_crf_filter(p, p, 1, 0, 8, 8, 1, 67.0, 3.0, p, p, 1 << 40, None) == -1
    assert lib.dg_crf_filter(None, p, 1, 3, 8, 8, 1, 67.0, 3.0, p, p, 1 << 40, None) == -1       # bilateral without image
    assert lib.dg_crf_filter(p, p, 1, 3, 8, 8, 1, 67.0, 0.0, p, p, 1 << 40, None) == -1
    assert lib.dg_crf_filter(p, p, 1, 3, 8, 8, 0, 1.0, 3.0, p, p, 100, None) == -3
    assert lib.dg_crf_filter(p, p, 1, 3, 4096, 4096, 1, 1e-3, 3.0, p, p, 1 << 40, None) == -2
    ends = (ctypes.c_int32 * 2)(3, 7)
    assert lib.dg_crf_unary(p, 1, 8, 4, 4, 8, 8, ends, 2, p, None) == -1               # ends do not reach C
    assert lib.dg_crf_unary(None, 1, 7, 4, 4, 8, 8, ends, 2, p, None) == -1
    bad = (ctypes.c_int32 * 2)(3, 6)
    assert lib.dg_crf_unary(p, 1, 7, 4, 4, 8, 8, bad, 2, p, None) == -1               # ends do not rise to C
    assert "group ends" in lib.dg_last_error().decode()
    assert lib.dg_segment_unary(p, None, 1, 8, 4, 4, p, None, 3, p, 4, 8, 8, 2.0, p, p, 10, None) == -3
    assert lib.dg_segment_unary(p, None, 1, 8, 4, 4, p, None, 0, p, 4, 8, 8, 2.0, p, p, 1 << 30, None) == -1


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from depthg_amd import ops, predict_and_score
    from depthg_amd.crf import batched_crf, dense_crf
    from depthg_amd.head import ClusterLookup
    img, U = torch.zeros(1, 3, 8, 8), torch.zeros(1, 7, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dense_crf(img, U, [3, 7])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.crf_filter(U, img, bilateral=True)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.crf_unary(torch.zeros(1, 7, 4, 4), 8, 8, [3, 7])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.segment_unary(torch.zeros(1, 8, 4, 4), torch.zeros(3, 8), None, torch.zeros(4, 8), 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        dense_crf(img[0], torch.zeros(7, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        batched_crf(img, torch.zeros(1, 7, 4, 4))
    with pytest.raises(ValueError, match="group ends"):
        ops.dense_crf(img, U, [3, 6])
    with pytest.raises(ValueError, match="group ends"):
        ops.crf_unary(torch.zeros(1, 7, 4, 4), 8, 8, [0, 7])
    with pytest.raises(ValueError):
        dense_crf(img, torch.zeros(7, 4, 4))
    linear, cluster = torch.nn.Conv2d(8, 5, 1), ClusterLookup(8, 7)
    code, label = torch.randn(2, 8, 4, 4), torch.zeros(2, 16, 16, dtype=torch.long)
    with pytest.raises(ValueError, match="img"):
        predict_and_score(code, label, linear, cluster, run_crf=True)
    with pytest.raises(ValueError, match="label size"):
        predict_and_score(code, label, linear, cluster, img=torch.zeros(2, 3, 16, 15), run_crf=True)
    with pytest.raises(RuntimeError, match="GPU"):
        predict_and_score(code, label, linear, cluster, img=torch.zeros(2, 3, 16, 16), run_crf=True)


def test_crf_kernels_use_no_scratch_and_no_flat_memory(tmp_path):
    """The audit of test_eval_cpu.py on dg_crf.hip (the sort and scan are rocPRIM's, in dg_crf_sort.hip)."""
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "depthg_amd", "csrc", "dg_crf.hip")
    out = tmp_path / "dg_crf.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    text = out.read_text()
    flat = [l.strip() for l in text.splitlines() if re.match(r"\s+flat_(load|store|atomic)", l)]
    assert not flat, f"dg_crf: FLAT memory instructions: {flat[:3]}"
    scratch = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    assert len(scratch) >= 20, scratch
    bad = {k: v for k, v in scratch.items() if v > 0}
    assert not bad, f"dg_crf: kernels with scratch (bytes per thread): {bad}"


def test_colour_chain_matches_torch():
    rng = np.random.default_rng(5)
    img = normalised_images(rng, 2, 31, 45)
    img[0, :, 0, :4] = torch.tensor([[-3.0, 5.0, float("nan"), 0.0]] * 3)         # outside [0, 255] after unnormalising: clamped
    for b in range(2):
        t = img[b].clone()
        for c, (m, s) in enumerate(zip([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])):
            t[c].mul_(s).add_(m)
        want = t.mul(255).clamp(0, 255).nan_to_num(0.0).byte().permute(1, 2, 0).numpy()[:, :, ::-1]
        assert np.array_equal(R.colour_image(img[b].numpy()), want)


def test_restated_message_is_symmetric_up_to_the_lattice_boundary():
    """<u, K~v> = <K~u, v> holds up to the lattice's boundary: the blur directions do not commute where neighbours are missing, so
    the restatement (like densecrf, which offers a transposed pass for that reason) is symmetric to ~5e-4 of |u| |K~v| here."""
    rng = np.random.default_rng(1)
    H, W = 37, 53
    img = normalised_images(rng, 1, H, W)[0].numpy()
    for lat in (R.gaussian_lattice(H, W), R.bilateral_lattice(img)):
        nrm = lat.norm()
        u, v = rng.random((H * W, 3)).astype(np.float32), rng.random((H * W, 3)).astype(np.float32)
        Kv, Ku = lat.message(v, nrm), lat.message(u, nrm)
        lhs, rhs = float((u * Kv).astype(np.float64).sum()), float((Ku * v).astype(np.float64).sum())
        assert abs(lhs - rhs) <= 2e-3 * np.linalg.norm(u) * np.linalg.norm(Kv), (lat.d, lhs, rhs)
        # the weights of a pixel's simplex sum to 1, and the constant field's message is close to 1 away from the image border
        assert np.allclose(lat.bary.sum(1), 1.0, atol=1e-5)


@pytest.mark.parametrize("zero", ["iterations", "weights"])
def test_restated_mean_field_without_pairwise_terms_is_the_softmax(zero):
    rng = np.random.default_rng(2)
    img = normalised_images(rng, 1, 11, 13)[0].numpy()
    U = rng.random((7, 11, 13)).astype(np.float32) * 4
    kw = dict(n_iter=0) if zero == "iterations" else dict(pos_w=0.0, bi_w=0.0)
    Q = R.dense_crf(img, U, [3, 7], **kw)
    want = np.concatenate([torch.softmax(-torch.from_numpy(U[:3]), 0).numpy(), torch.softmax(-torch.from_numpy(U[3:]), 0).numpy()])
    assert np.allclose(Q, want, atol=1e-6)


def test_restated_unary_matches_the_reference_formula():
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((5, 6, 7)).astype(np.float32) * 4
    U = R.unary_from_logits(logits, 6, 7)
    p = torch.softmax(torch.from_numpy(logits), 0).numpy()
    assert np.array_equal(U, -np.log(np.clip(p, np.float32(1e-5), np.float32(1.0))))


def test_against_pydensecrf():
    """The restatement against pydensecrf itself (src/crf.py's chain), where that library is installed."""
    dcrf = pytest.importorskip("pydensecrf.densecrf")
    rng = np.random.default_rng(4)
    H, W, C = 23, 29, 5
    img = normalised_images(rng, 1, H, W)[0].numpy()
    U = R.unary_from_logits(rng.standard_normal((C, 8, 9)).astype(np.float32) * 3, H, W)
    d = dcrf.DenseCRF2D(W, H, C)
    d.setUnaryEnergy(np.ascontiguousarray(U.reshape(C, -1)))
    d.addPairwiseGaussian(sxy=1, compat=3)
    d.addPairwiseBilateral(sxy=67, srgb=3, rgbim=R.colour_image(img), compat=4)
    want = np.array(d.inference(10)).reshape(C, H, W)
    assert np.abs(R.dense_crf(img, U) - want).max() <= 1e-4


def _runs(img):
    """The splat runs of one image's bilateral lattice, in sorted-key order: the restatement numbers its vertices by their packed
    key, first coordinate most significant, as dg_crf.hip's sort does."""
    return np.bincount(R.bilateral_lattice(img.numpy()).offsets.ravel())


def test_flat_region_images_give_long_splat_runs_and_noise_does_not():
    """Why flat_region_images exists: on noise no splat run is longer than 4 entries, so a run crosses one tile boundary at the
    most: k_crf_splat_tail never sums a whole tile and k_crf_splat_head never adds two partial sums.  On flat regions every image
    has runs that cross at least two boundaries wherever they start."""
    src = open(os.path.join(ROOT, "depthg_amd", "csrc", "dg_crf.hip")).read()
    assert re.search(rf"#define CRF_TILE {CRF_TILE}\b", src)
    assert _runs(normalised_images(np.random.default_rng(10), 1, 37, 53)[0]).max() <= 4
    assert any((6 * H * W) % CRF_TILE for H, W in FLAT_SHAPES)          # a last tile that is cut short by the end of its image
    for H, W in FLAT_SHAPES:
        img = flat_region_images(np.random.default_rng(FLAT_SEED), 4, H, W)
        assert img.shape == (4, 3, H, W) and img.dtype == torch.float32
        assert len({img[b].numpy().tobytes() for b in range(4)}) == 4
        for b in range(4):
            bgr = R.colour_image(img[b].numpy())
            assert (bgr == 255).all(2).sum() >= H * W // 5 and (bgr == 0).all(2).sum() >= H * W // 8       # exactly white, exactly black
            runs = _runs(img[b])
            assert runs.max() >= 4 * CRF_TILE, (H, W, b, runs.max())
            assert (runs > 2 * CRF_TILE).sum() >= 10, (H, W, b, (runs > 2 * CRF_TILE).sum())
            if b < 2:                                                   # the image's last run continues into its last tiles
                assert runs[-1] > 2 * CRF_TILE, (H, W, b, runs[-1])
        one = flat_region_images(np.random.default_rng(FLAT_SEED), 2, H, W, single_colour=True)
        assert not torch.equal(one[0], one[1])
        for b in range(2):
            assert len(np.unique(R.colour_image(one[b].numpy()).reshape(-1, 3), axis=0)) == 1
            runs = _runs(one[b])
            assert runs.max() >= 4 * CRF_TILE and (runs > 2 * CRF_TILE).sum() >= 10, (H, W, b, runs)


@pytest.mark.parametrize("single_colour", [False, True])
def test_restated_message_in_fp32_agrees_with_float64_accumulation_on_flat_images(single_colour):
    """The restatement sums a run of thousands of entries in fp32, in sorted order.  Against the same lattice accumulated in
    float64 (splat, blur, slice and norm) its message moves by 2e-7 .. 3e-7 of the largest value on these images (bound: 1e-6),
    so the order of summation does not limit the 1e-5 bound of the GPU filter tests."""
    for H, W in FLAT_SHAPES:
        rng = np.random.default_rng(42)
        img = flat_region_images(np.random.default_rng(FLAT_SEED), 1, H, W, single_colour=single_colour)[0].numpy()
        lat = R.bilateral_lattice(img)
        vals = rng.random((H * W, 6)).astype(np.float32)
        m32, m64 = lat.message(vals), lat.message(vals, dtype=np.float64)
        assert m32.dtype == np.float32 and m64.dtype == np.float64
        rel = np.abs(m32 - m64).max() / np.abs(m64).max()
        print(f"fp32 against float64 message, {H} x {W}, single_colour={single_colour}: {rel:.2e}")
        assert rel <= 1e-6, (H, W, rel)
