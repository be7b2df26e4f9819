"""The contrastive CRF loss term on the GPU (dg_crf_loss.hip through ops.crf_loss_forward / crf_loss_backward and
ContrastiveCRFLoss.mean_loss): loss and d code against the float64 restatement of the whole chain (tests/crf_loss_reference.py) with
the same chain in float32 torch on the GPU as the yardstick, the bilinear pick, zero code vectors, determinism, the complete write of
d code, and cfg.crf_weight in training_step.

MARGIN: the kernels' errors may be at most MARGIN x the yardstick's - 2, what tests/adam_reference.py holds for the fused Adam.
scripts/crf_loss_parity.py runs measure() over CASES and writes the ratios to profiles/crf_loss_parity.md.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import crf_loss_reference as R

MARGIN = 2.0
# Where the true d code vanishes - one sample, all samples on one pixel, samples too far apart for the nearly diagonal default kernel:
# the loss is then constant under the normalisation - a relative error compares rounding noise with rounding noise.  A case whose
# true gradient lies below one float32 spacing (2^-23) of R.gradient_scale, what the gradient would be if nothing cancelled, is held
# to an absolute bound as well: the kernels' d code may not exceed NOISE_ULPS spacings of that scale.  8: the row sums G_a are float32
# chains of up to n / 4 = 250 terms, whose roundings walk sqrt(250) / 2 = 8 half-spacings; everything behind G is a projection in fp64.
NOISE_ULPS = 8.0
ULP32 = 2.0 ** -23
SETS = {"default": R.DEFAULT_SET, "dense": R.DENSE_SET}
# name: (D, (h, w), (H, W), size, n, coordinates)
SHAPES = {
    "n1": (5, (4, 4), (32, 32), 56, 1, "random"),
    "nonsquare": (5, (7, 9), (40, 72), 56, 7, "random"),
    "mid": (70, (28, 28), (224, 224), 56, 257, "random"),
    "wide": (128, (14, 14), (112, 112), 56, 64, "random"),
    "full": (70, (28, 28), (224, 224), 56, 1000, "random"),
    "down": (33, (6, 6), (20, 20), 8, 40, "random"),            # downscaling and tiny maps
    "nonsquare_onepixel": (5, (7, 9), (40, 72), 56, 7, "onepixel"),
    "nonsquare_corners": (5, (7, 9), (40, 72), 56, 4, "corners"),
    "nonsquare_twice": (5, (7, 9), (40, 72), 56, 14, "twice"),
    "mid_onepixel": (70, (28, 28), (224, 224), 56, 257, "onepixel"),
    "mid_corners": (70, (28, 28), (224, 224), 56, 4, "corners"),
    "mid_twice": (70, (28, 28), (224, 224), 56, 514, "twice"),
}
CASES = [(shape, sset) for shape in SHAPES for sset in SETS]
B = 2
# More partial sums than the 256 threads of k_loss_reduce, so that its strided loop runs twice.  k_crfl_pair leaves one partial per
# image and 64 R samples, and R = 1 only above 72 channels (with D = 3 a block takes 128 samples and the same n leaves 135 partials;
# D = 3 also lets interpolated code vectors fall below the 0.1 the cases keep): 5 images x ceil(3400 / 64) = 270.
# (The name sorts behind the others: inputs() seeds by the sorted position.)
SHAPES["wraps"] = (73, (8, 8), (16, 16), 64, 3400, "random")
BATCH = {"wraps": 5}                                          # images, where not B
CASES += [("wraps", "dense")]


def make_coords(kind, size, n, gen):
    if kind == "onepixel":
        return torch.tensor([[size // 3] * n, [size - 2] * n])
    if kind == "corners":
        return torch.tensor([[0, 0, size - 1, size - 1], [0, size - 1, 0, size - 1]])
    if kind == "twice":
        half = torch.stack([torch.randint(0, size, (n // 2,), generator=gen), torch.randint(0, size, (n // 2,), generator=gen)])
        return torch.cat([half, half], 1)
    return torch.stack([torch.randint(0, size, (n,), generator=gen), torch.randint(0, size, (n,), generator=gen)])


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(img, code, coords) on the CPU: a normalised-RGB-like image, a code map whose interpolated vectors keep a norm >= 0.1."""
    D, (h, w), (H, W), size, n, kind = SHAPES[shape]
    gen = torch.Generator().manual_seed(sorted(SHAPES).index(shape) + 100)
    Bn = BATCH.get(shape, B)
    img = (torch.randn(Bn, 3, H, W, generator=gen) * 1.1).clamp(-2.1, 2.6)
    code = torch.randn(Bn, D, h, w, generator=gen) + 0.6
    return img, code, make_coords(kind, size, n, gen)


@functools.lru_cache(maxsize=None)
def truth(shape, sset):
    """The float64 restatement, once per case: (loss, d code, mean |sims K|, S, g) - shared by the tests, never modified."""
    img, code, coords = inputs(shape)
    return R.chain(img, code, coords, SHAPES[shape][3], SETS[sset])


def yardstick(shape, sset, dev):
    """resize + norm + the compatibility forward + .mean() + autograd in float32 torch on the GPU."""
    from depthg_amd import ContrastiveCRFLoss
    img, code, coords = inputs(shape)
    size, n = SHAPES[shape][3], SHAPES[shape][4]
    c = code.to(dev).requires_grad_(True)
    resize = lambda t: F.interpolate(t, (size, size), mode="bilinear", align_corners=False)
    fn = ContrastiveCRFLoss(n, **SETS[sset])
    loss = fn(resize(img.to(dev)), F.normalize(resize(c), dim=1, eps=1e-10), coords=coords.to(dev)).mean()
    loss.backward()
    return float(loss.detach().double()), c.grad.double().cpu()


def kernel(shape, sset, dev):
    from depthg_amd import ContrastiveCRFLoss
    img, code, coords = inputs(shape)
    size, n = SHAPES[shape][3], SHAPES[shape][4]
    c = code.to(dev).requires_grad_(True)
    loss = ContrastiveCRFLoss(n, **SETS[sset]).mean_loss(img.to(dev), c, size=size, coords=coords.to(dev))
    loss.backward()
    return float(loss.detach().double()), c.grad.double().cpu()


def measure(shape, sset, dev):
    """The figures of one case: loss errors (absolute, over the mean |sims K|) and d code errors (relative L2) of the kernels and of
    the yardstick against the float64 restatement."""
    want_loss, want_grad, mean_abs, _, _ = truth(shape, sset)
    k_loss, k_grad = kernel(shape, sset, dev)
    y_loss, y_grad = yardstick(shape, sset, dev)
    rel = lambda g: float((g - want_grad).norm() / want_grad.norm())
    img, code, coords = inputs(shape)
    gscale = R.gradient_scale(img, code, coords, SHAPES[shape][3], SETS[sset])
    return {"grad_scale": gscale, "grad_true_max": float(want_grad.abs().max()), "grad_kernel_max": float(k_grad.abs().max()),
            "loss": want_loss, "kernel_loss": k_loss, "mean_abs": mean_abs,
            "loss_err_kernel": abs(k_loss - want_loss) / mean_abs, "loss_err_yard": abs(y_loss - want_loss) / mean_abs,
            "loss_rel_kernel": abs(k_loss - want_loss) / abs(want_loss),
            "grad_err_kernel": rel(k_grad), "grad_err_yard": rel(y_grad)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,sset", CASES)
def test_loss_and_gradient_within_the_yardsticks_margin(shape, sset, dev):
    img, code, _ = inputs(shape)
    size = SHAPES[shape][3]
    assert float(R.resize(code.double(), size).square().sum(1).sqrt().min()) >= 0.1       # every interpolated code vector
    assert float(img.min()) >= -2.2 and float(img.max()) <= 2.7
    m = measure(shape, sset, dev)
    print(f"{shape}/{sset}: loss {m['loss']:.9e} kernel {m['kernel_loss']:.9e} | loss err kernel {m['loss_err_kernel']:.3e} yardstick "
          f"{m['loss_err_yard']:.3e} | d code rel-L2 kernel {m['grad_err_kernel']:.3e} yardstick {m['grad_err_yard']:.3e}")
    assert m["loss_rel_kernel"] <= 1e-4
    assert m["loss_err_kernel"] <= MARGIN * m["loss_err_yard"], m
    assert m["grad_err_kernel"] <= MARGIN * m["grad_err_yard"], m
    if m["grad_true_max"] < ULP32 * m["grad_scale"]:           # the true gradient vanishes: the ratio above holds noise against noise
        print(f"{shape}/{sset}: true |d code| <= {m['grad_true_max']:.3e}, kernel <= {m['grad_kernel_max']:.3e}, scale {m['grad_scale']:.3e}")
        assert m["grad_kernel_max"] <= NOISE_ULPS * ULP32 * m["grad_scale"], m


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["down", "nonsquare", "nonsquare_corners"])
def test_bilinear_pick_and_norm_in_the_workspace(shape, dev):
    """S and g as k_crfl_sample left them equal norm(resize(code)) and resize(img) at the coordinates."""
    from depthg_amd import ops
    img, code, coords = inputs(shape)
    D, _, _, size, n, _ = SHAPES[shape]
    loss, ws = ops.crf_loss_forward(code.to(dev), img.to(dev), coords.to(dev), size, **R.DEFAULT_SET)
    sec = ops.crf_loss_workspace_sections(ws, B, D, n)
    resize = lambda t: F.interpolate(t, (size, size), mode="bilinear", align_corners=False)
    ys, xs = coords[0].to(dev), coords[1].to(dev)
    want_S = F.normalize(resize(code.to(dev)), dim=1, eps=1e-10)[:, :, ys, xs].permute(0, 2, 1)
    want_g = resize(img.to(dev))[:, :, ys, xs].permute(0, 2, 1)
    assert float((sec["S"][:, :, :D] - want_S).abs().max()) <= 1e-6
    assert float((sec["g"][:, :, :3] - want_g).abs().max()) <= 1e-6
    assert not bool(sec["S"][:, :, D:].any()) and not bool(sec["g"][:, :, 3].any())
    want_norm = resize(code.to(dev)).square().sum(1).sqrt()[:, ys, xs]
    assert torch.allclose(sec["norm"], want_norm, rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_zero_code_vectors_give_a_finite_forward(dev):
    from depthg_amd import ContrastiveCRFLoss, ops
    gen = torch.Generator().manual_seed(3)
    img, code = torch.randn(B, 3, 8, 8, generator=gen).to(dev), torch.randn(B, 6, 4, 4, generator=gen).to(dev)
    code[:, :, 1, 2] = 0                                       # size == h == w: the resize is the identity, sample 0 IS that pixel
    coords = torch.tensor([[1, 0, 3, 2, 1], [2, 0, 3, 1, 1]], device=dev)
    loss, ws = ops.crf_loss_forward(code, img, coords, 4, **R.DENSE_SET)
    sec = ops.crf_loss_workspace_sections(ws, B, 6, 5)
    assert bool(torch.isfinite(loss)) and not bool(sec["S"][:, 0].any()) and not bool(sec["norm"][:, 0].any())
    assert bool(torch.isfinite(sec["S"]).all()) and bool(torch.isfinite(sec["G"]).all())
    want, _, mean_abs, _, _ = R.chain(img, code, coords, 4, R.DENSE_SET)
    assert abs(float(loss) - want) <= 1e-5 * mean_abs
    c = code.clone().requires_grad_(True)
    ContrastiveCRFLoss(5, **R.DENSE_SET).mean_loss(img, c, size=4, coords=coords).backward()
    assert bool(torch.isfinite(c.grad).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["mid", "down"])
def test_two_calls_give_the_same_bits_and_d_code_is_written_completely(shape, dev):
    from depthg_amd import ops
    img, code, coords = (t.to(dev) for t in inputs(shape))
    D, (h, w), _, size, n, _ = SHAPES[shape]
    runs = []
    for _ in range(2):
        loss, ws = ops.crf_loss_forward(code, img, coords, size, **R.DENSE_SET)
        out = torch.full((B, D, h, w), float("nan"), device=dev)
        ops.crf_loss_backward(ws, coords, (B, D, h, w), size, torch.tensor(0.75, device=dev), out=out)
        runs.append((loss.clone(), out))
    assert not bool(torch.isnan(runs[0][1]).any())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the upstream gradient is a factor
    once = ops.crf_loss_backward(ws, coords, (B, D, h, w), size, torch.tensor(1.0, device=dev))
    assert torch.allclose(runs[1][1], once * 0.75, rtol=1e-6, atol=0)


def _batch(dev, seed=0, hw=32, n_classes=5):
    g = torch.Generator().manual_seed(seed)
    return {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
            "label": torch.randint(-1, n_classes, (B, hw, hw), generator=g).to(dev),
            "depth": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev),
            "depth_pos": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev)}


def _segmenter(dev, **over):
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(4)
    m = UnsupervisedSegmenter(5, default_segmenter_cfg(res=32, crf_samples=64, correspondence_weight=0.0, **over)).to(dev)
    m.train()
    return m


@pytest.mark.gpu
def test_training_step_adds_the_term_under_crf_weight(dev):
    m = _segmenter(dev, crf_weight=0.5)
    head0 = [p.detach().clone() for p in m.head_parameters()]
    torch.manual_seed(9)
    loss, logs = m.training_step(_batch(dev), 0)
    assert "loss/crf" in logs and bool(torch.isfinite(loss))
    want = float(logs["loss/linear"]) + float(logs["loss/cluster"]) + 0.5 * float(logs["loss/crf"])
    assert abs(float(logs["loss/total"]) - want) <= 4e-7 * (abs(float(logs["loss/linear"])) + abs(float(logs["loss/cluster"])) + abs(float(logs["loss/crf"])))
    assert float(logs["loss/crf"]) != 0.0
    assert any(not torch.equal(a, b.detach()) for a, b in zip(head0, m.head_parameters()))
    # the logged value is the term itself on the draw the step made
    m2 = _segmenter(dev, crf_weight=0.5)
    torch.manual_seed(9)
    _, logs2 = m2.training_step(_batch(dev), 0)
    assert torch.equal(logs2["loss/crf"], logs["loss/crf"])


@pytest.mark.gpu
def test_training_step_without_crf_weight_draws_and_launches_nothing(dev, monkeypatch):
    from depthg_amd import crf_loss, ops

    def run(strip):
        m = _segmenter(dev, crf_weight=0.0)
        if strip:
            m.crf_loss_fn = None                                # any use of the term would raise
        head0 = [p.detach().clone() for p in m.head_parameters()]
        torch.manual_seed(9)
        loss, logs = m.training_step(_batch(dev), 0)
        torch.cuda.synchronize()
        return m, head0, loss, logs, torch.get_rng_state(), torch.cuda.get_rng_state(dev)

    # The two patches carry the assertion: with crf_weight = 0 neither the term's one draw routine nor its one launch routine may be
    # reached.  The comparison of the generator states below is between two runs of this code (the second without the loss object),
    # not against the parent commit: it would not see a draw made by some other path in both.
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the CRF term ran with crf_weight = 0"))
    monkeypatch.setattr(ops, "crf_loss_forward", boom)
    monkeypatch.setattr(crf_loss, "draw_coords", boom)
    m, head0, loss, logs, cpu_state, gpu_state = run(False)
    assert "loss/crf" not in logs
    assert all(torch.equal(a, b.detach()) for a, b in zip(head0, m.head_parameters()))
    _, _, loss_s, logs_s, cpu_s, gpu_s = run(True)
    assert torch.equal(cpu_state, cpu_s) and torch.equal(gpu_state, gpu_s)              # no extra draws
    assert torch.equal(loss, loss_s) and set(logs) == set(logs_s)
