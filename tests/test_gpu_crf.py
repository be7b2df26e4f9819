"""The dense CRF on the GPU (dg_crf_filter, dg_dense_crf, dg_crf_unary, dg_segment_unary through depthg_amd.ops, depthg_amd.crf and
predict_and_score(run_crf=True) / evaluate_batch(run_crf=True)) against the numpy restatement of tests/crf_reference.py.

Images are T.Normalize of random uint8 images, so many colour values sit within rounding of a truncation boundary: one colour level
off moves a bilateral feature by 1/3 and breaks the 1e-5 bound of the filter tests.  Bounds: filter relative error <= 1e-5;
mean field max|dQ| <= 1e-4 (at 320 x 320: on all but 0.01 % of the pixels, see the test), predictions equal except where the reference's top-2 gap in Q is below 1e-3 and on >= 99.9 % of pixels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crf_reference as R
from test_crf_cpu import normalised_images

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def check_preds(got, Q_ref, ends):
    """got (G,H,W) int64 per-group arg-maxes; Q_ref (C,H,W) the restatement's Q."""
    start, worst = 0, 0
    for g, end in enumerate(ends):
        q = torch.from_numpy(Q_ref[start:end])
        want = q.argmax(0)
        top = q.topk(min(2, end - start), dim=0).values
        gap = (top[0] - top[1]) if end - start > 1 else torch.full_like(top[0], 1.0)
        diff = got[g].cpu() != want
        assert not (diff & (gap >= 1e-3)).any(), int((diff & (gap >= 1e-3)).sum())
        assert int(diff.sum()) <= 1e-3 * diff.numel()
        worst = max(worst, int(diff.sum()))
        start = end
    return worst


@pytest.mark.parametrize("bilateral", [False, True])
def test_crf_filter_matches_restatement(bilateral):
    from depthg_amd import ops
    rng = np.random.default_rng(10)
    B, C, H, W = 2, 6, 37, 53
    img = normalised_images(rng, B, H, W)
    vals = torch.from_numpy(rng.random((B, C, H, W)).astype(np.float32))
    got = ops.crf_filter(vals.to(DEV), img.to(DEV), bilateral=bilateral, sxy=67.0 if bilateral else 1.0, srgb=3.0).cpu().numpy()
    for b in range(B):
        lat = R.bilateral_lattice(img[b].numpy()) if bilateral else R.gaussian_lattice(H, W)
        want = lat.message(vals[b].numpy().reshape(C, -1).T).T.reshape(C, H, W)
        rel = np.abs(got[b] - want).max() / np.abs(want).max()
        assert rel <= 1e-5, rel


def test_bilateral_filter_of_one_hot_fields_sees_the_uint8_colours():
    """A one-hot field (the Q of a confident pixel) through the bilateral kernel: a pixel whose colour is one level off moves its
    feature by 1/3 and changes its weights far beyond 1e-5."""
    from depthg_amd import ops
    rng = np.random.default_rng(11)
    B, C, H, W = 1, 4, 40, 40
    img = normalised_images(rng, B, H, W)
    lab = rng.integers(0, C, (H, W))
    onehot = np.eye(C, dtype=np.float32)[lab].transpose(2, 0, 1)[None]
    got = ops.crf_filter(torch.from_numpy(onehot).to(DEV), img.to(DEV), bilateral=True, sxy=67.0, srgb=3.0).cpu().numpy()[0]
    want = R.bilateral_lattice(img[0].numpy()).message(onehot[0].reshape(C, -1).T).T.reshape(C, H, W)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def test_crf_filter_symmetry_matches_the_restatement():
    """<u, K~v> - <K~u, v>: zero in the interior of the lattice, not at its boundary (the blur directions do not commute where
    neighbours are missing).  The GPU's asymmetry must be the restatement's, to 2e-6 of |u| |K~v|, against an asymmetry of
    2e-5 .. 5e-4 of it here: a wrong normalisation, weight or neighbour moves it far more."""
    from depthg_amd import ops
    rng = np.random.default_rng(12)
    H, W = 37, 53
    img = normalised_images(rng, 1, H, W)
    u, v = (rng.random((1, 3, H, W)).astype(np.float32) for _ in range(2))
    for bil in (False, True):
        kw = dict(bilateral=bil, sxy=67.0 if bil else 1.0, srgb=3.0)
        Kv = ops.crf_filter(torch.from_numpy(v).to(DEV), img.to(DEV), **kw).cpu().double().numpy()
        Ku = ops.crf_filter(torch.from_numpy(u).to(DEV), img.to(DEV), **kw).cpu().double().numpy()
        scale = np.linalg.norm(u) * np.linalg.norm(Kv)
        asym = ((u * Kv).sum() - (Ku * v).sum()) / scale
        lat = R.bilateral_lattice(img[0].numpy()) if bil else R.gaussian_lattice(H, W)
        uf, vf = u[0].reshape(3, -1).T, v[0].reshape(3, -1).T
        nrm = lat.norm()
        asym_ref = (float((uf.astype(np.float64) * lat.message(vf, nrm)).sum())
                    - float((lat.message(uf, nrm).astype(np.float64) * vf).sum())) / scale
        print(f"symmetry {'bilateral' if bil else 'Gaussian'}: asymmetry {asym:.3e}, restatement {asym_ref:.3e}")
        assert abs(asym_ref) > 1e-5 and abs(asym - asym_ref) <= 2e-6, (asym, asym_ref)


def _dense_case(rng, B, C_ends, H, W, h, w, images=normalised_images):
    from depthg_amd import ops
    img = images(rng, B, H, W)
    logits = torch.from_numpy(rng.standard_normal((B, C_ends[-1], h, w)).astype(np.float32) * 3)
    U = ops.crf_unary(logits.to(DEV), H, W, C_ends)
    U_ref = np.stack([R.unary_from_logits(logits[b].numpy(), H, W, C_ends) for b in range(B)])
    assert np.abs(U.cpu().numpy() - U_ref).max() <= 1e-5
    return img, U, U_ref


@pytest.mark.parametrize("shape", ["small", "eval320"])
def test_dense_crf_matches_restatement(shape):
    from depthg_amd import ops
    rng = np.random.default_rng(13)
    if shape == "small":
        B, ends, H, W, h, w = 2, [3, 7], 37, 53, 10, 14
    else:
        B, ends, H, W, h, w = 1, [27, 54], 320, 320, 40, 40
    img, U, U_ref = _dense_case(rng, B, ends, H, W, h, w)
    q, preds = ops.dense_crf(img.to(DEV), U, ends, return_q=True, return_preds=True)
    q2, preds2 = ops.dense_crf(img.to(DEV), U, ends, return_q=True, return_preds=True)
    assert torch.equal(q, q2) and torch.equal(preds, preds2)                        # determinism
    q, preds = q.cpu().numpy(), preds.cpu()
    errs = []
    for b in range(B):
        Q_ref = R.dense_crf(img[b].numpy(), U_ref[b], ends)
        px = np.abs(q[b] - Q_ref).max(0)
        errs.append(float(px.max()))
        if shape == "small":
            assert px.max() <= 1e-4, px.max()
        else:
            # Ten iterations amplify rounding near decision boundaries: at this size a 1-ulp perturbation of U moves the
            # restatement's own Q by up to 2.2e-4 (3 pixels above 1e-4).  So 1e-4 holds on all but 0.01 % of the pixels, 1e-3 on all.
            assert (px > 1e-4).sum() <= 1e-4 * px.size and px.max() <= 1e-3, ((px > 1e-4).sum(), px.max())
        nd = check_preds(preds[:, b], Q_ref, ends)
        print(f"dense_crf {shape} image {b}: max|dQ| = {px.max():.3e}, pixels above 1e-4: {int((px > 1e-4).sum())}, "
              f"differing predictions: {nd}")


def test_dense_crf_chunks_and_zero_iterations():
    """A workspace of one image (chunks of 1) gives the bits of the whole batch at once; n_iter = 0 gives softmax(-U)."""
    from depthg_amd import _lib, ops
    rng = np.random.default_rng(14)
    ends = [3, 7]
    img, U, _ = _dense_case(rng, 3, ends, 19, 23, 19, 23)
    one = _lib.load().dg_crf_workspace_bytes(1, 19, 23, 8, 3)
    q_all, p_all = ops.dense_crf(img.to(DEV), U, ends, return_preds=True)
    q_one, p_one = ops.dense_crf(img.to(DEV), U, ends, return_preds=True, workspace_budget=one)
    assert torch.equal(q_all, q_one) and torch.equal(p_all, p_one)
    q0, _ = ops.dense_crf(img.to(DEV), U, ends, n_iter=0)
    want = torch.cat([torch.softmax(-U[:, :3], 1), torch.softmax(-U[:, 3:], 1)], 1)
    assert (q0 - want).abs().max() <= 1e-6


def test_crf_module_mirrors_src_crf():
    from depthg_amd.crf import batched_crf, dense_crf
    rng = np.random.default_rng(15)
    img = normalised_images(rng, 2, 24, 30)
    logits = torch.from_numpy(rng.standard_normal((2, 5, 6, 8)).astype(np.float32) * 2)
    out = batched_crf(img.to(DEV), logits.to(DEV))
    assert out.shape == (2, 5, 24, 30) and out.is_cuda
    one = dense_crf(img[1].to(DEV), logits[1].to(DEV))
    assert torch.equal(one, out[1])
    want = R.dense_crf(img[1].numpy(), R.unary_from_logits(logits[1].numpy(), 24, 30))
    assert np.abs(one.cpu().numpy() - want).max() <= 1e-4


def ref_log_probs(code, lin_w, lin_b, clusters, H, W, code_flip=None):
    """fp64 chain of src/eval_segmentation.py:150-160: (linear, cluster) log-probabilities (B,n,H,W), (B,m,H,W)."""
    c = code.double()
    if code_flip is not None:
        c = (c + code_flip.double().flip(dims=[3])) / 2
    up = F.interpolate(c, (H, W), mode="bilinear", align_corners=False)
    lin = F.conv2d(up, lin_w.double()[:, :, None, None], lin_b.double())
    inner = torch.einsum("bchw,nc->bnhw", F.normalize(up, dim=1), F.normalize(clusters.double(), dim=1))
    return torch.log_softmax(lin, 1), torch.log_softmax(inner * 2, 1)


def _eval_case(seed, B=2, D=16, h=8, w=10, H=40, W=48, n=5, m=6, images=normalised_images):
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    code, code_flip = torch.randn(B, D, h, w, generator=g), torch.randn(B, D, h, w, generator=g)
    lin_w, lin_b, clusters = torch.randn(n, D, generator=g), torch.randn(n, generator=g), torch.randn(m, D, generator=g)
    label = torch.randint(-1, n + 1, (B, H, W), generator=g)
    img = images(rng, B, H, W)
    return code, code_flip, lin_w, lin_b, clusters, label, img


def check_run_crf_chain(case, flip):
    """predict_and_score(run_crf=True) on one _eval_case against the reference's chain: the unary, then the per-probe CRF's
    predictions.  Returns the probes, the metrics it fed and the predictions."""
    from depthg_amd import ops, predict_and_score
    from depthg_amd.metrics import UnsupervisedMetrics
    from test_gpu_eval import make_probes
    code, code_flip, lin_w, lin_b, clusters, label, img = case
    B, _, _, _ = code.shape
    n, m, H, W = lin_w.shape[0], clusters.shape[0], label.shape[-2], label.shape[-1]
    cf = code_flip if flip else None
    # the eval-route unary against the fp64 head chain's log-probabilities fed to the reference's unary
    U = ops.segment_unary(code.to(DEV), lin_w.to(DEV), lin_b.to(DEV), clusters.to(DEV), H, W,
                          code_flip=cf.to(DEV) if flip else None)
    lp, cp = ref_log_probs(code, lin_w, lin_b, clusters, H, W, cf)
    U_ref = [np.concatenate([R.unary_from_logits(lp[b].float().numpy(), H, W), R.unary_from_logits(cp[b].float().numpy(), H, W)])
             for b in range(B)]
    assert np.abs(U.cpu().numpy() - np.stack(U_ref)).max() <= 1e-4
    linear, cluster = make_probes(lin_w.to(DEV), lin_b.to(DEV), clusters.to(DEV))
    lm, cm = UnsupervisedMetrics("final/linear/", n, 0, False), UnsupervisedMetrics("final/cluster/", n, m - n, True)
    pl, pc = predict_and_score(code.to(DEV), label.to(DEV), linear, cluster, lm, cm, code_flip=cf.to(DEV) if flip else None,
                               n_store=B, img=img.to(DEV), run_crf=True)
    # the reference runs the CRF once per probe
    for b in range(B):
        Q_lin = R.dense_crf(img[b].numpy(), U_ref[b][:n])
        Q_clu = R.dense_crf(img[b].numpy(), U_ref[b][n:])
        check_preds(torch.stack([pl[b], pc[b]]), np.concatenate([Q_lin, Q_clu]), [n, n + m])
    return linear, cluster, lm, cm, pl, pc


@pytest.mark.parametrize("flip", [False, True])
def test_predict_and_score_run_crf_matches_reference_chain(flip):
    from depthg_amd import predict_and_score
    from depthg_amd.metrics import UnsupervisedMetrics
    code, code_flip, lin_w, lin_b, clusters, label, img = case = _eval_case(21 + flip)
    B, n, m = code.shape[0], lin_w.shape[0], clusters.shape[0]
    cf = code_flip if flip else None
    linear, cluster, lm, cm, pl, pc = check_run_crf_chain(case, flip)
    # the metrics' counts are the counts of the returned predictions
    lm2, cm2 = UnsupervisedMetrics("a/", n, 0, False), UnsupervisedMetrics("b/", n, m - n, True)
    lm2.update(pl, label.to(DEV))
    cm2.update(pc, label.to(DEV))
    assert torch.equal(lm.stats, lm2.stats) and torch.equal(cm.stats, cm2.stats)
    # n_store: the first images' predictions
    pl1, pc1 = predict_and_score(code.to(DEV), label.to(DEV), linear, cluster, code_flip=cf.to(DEV) if flip else None, n_store=1,
                                 img=img.to(DEV), run_crf=True)
    assert torch.equal(pl1, pl[:1]) and torch.equal(pc1, pc[:1])
    # run_crf=False is the previous scoring
    a = predict_and_score(code.to(DEV), label.to(DEV), linear, cluster, code_flip=cf.to(DEV) if flip else None, n_store=B)
    b_ = predict_and_score(code.to(DEV), label.to(DEV), linear, cluster, code_flip=cf.to(DEV) if flip else None, n_store=B,
                           img=img.to(DEV), run_crf=False)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])


def test_evaluate_batch_run_crf():
    from depthg_amd.evaluation import predict_and_score
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(6)
    cfg = default_segmenter_cfg(dim=70, extra_clusters=2)
    model = UnsupervisedSegmenter(27, cfg).to(DEV)
    model.eval()
    rng = np.random.default_rng(30)
    img = normalised_images(rng, 2, 112, 112).to(DEV)
    label = torch.randint(-1, 28, (2, 112, 112), device=DEV)
    lp, cp = model.evaluate_batch({"img": img, "label": label}, flip=True, run_crf=True)
    assert lp.shape == (2, 112, 112) and cp.shape == (2, 112, 112)
    code, code_flip = model._eval_mode_codes(img, True)
    wl, wc = predict_and_score(code, label, model.linear_probe, model.cluster_probe, code_flip=code_flip, n_store=2, img=img,
                               run_crf=True)
    assert torch.equal(lp, wl) and torch.equal(cp, wc)
    assert int(model.test_linear_metrics.stats.sum()) == int(((label >= 0) & (label < 27)).sum())
    with pytest.raises(ValueError, match="label size"):
        predict_and_score(code, label[:, :, :100], model.linear_probe, model.cluster_probe, img=img, run_crf=True)
