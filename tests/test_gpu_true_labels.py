"""cfg.use_true_labels on the GPU: k_label_onehot against the CPU route (the reference's torch chain) bit for bit, dg_fps_coords_large
against dg_fps_coords bit for bit and against the oracle's FPS above the old limit, the loss on one-hot signals against the
reference's fixtures (tests/golden/true_labels_*.npz, scripts/make_true_labels_fixtures.py) within the bounds
tests/test_gpu_parity.py::test_golden_forward_backward holds its sampled golden cases to, and one training step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import cfg_from_fixture, load_golden  # noqa: E402
from label_onehot_reference import ONEHOT_SHAPES, one_hot_signal, random_labels  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


# ---- k_label_onehot ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,H,W", ONEHOT_SHAPES)
def test_onehot_kernel_equals_cpu_route(B, K, H, W, dev):
    from depthg_amd import ops
    label, label_pos = random_labels(21, B, K - 1, H, W), random_labels(22, B, K - 1, H, W)
    want, want_pos = ops.label_onehot(label, K - 1), ops.label_onehot(label_pos, K - 1)
    got = ops.label_onehot(label.to(dev), K - 1)
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got.cpu(), want)
    # the paired launch: two views of one allocation, in order
    a, b = ops.label_onehot(label.to(dev), K - 1, label_pos.to(dev))
    assert torch.equal(a.cpu(), want) and torch.equal(b.cpu(), want_pos)
    assert a.is_contiguous() and b.is_contiguous() and b.data_ptr() == a.data_ptr() + a.numel() * 4
    assert torch.equal(ops.label_onehot(label.unsqueeze(1).to(dev), K - 1).cpu(), want)          # (B,1,H,W)
    assert torch.equal(ops.label_onehot(label.to(dev), K - 1, check=False).cpu(), want)


@pytest.mark.parametrize("H,W", [(20, 68), (5, 7)])
def test_onehot_kernel_constant_maps_and_poison(H, W, dev, monkeypatch):
    from depthg_amd import ops
    n = 27
    monkeypatch.setattr(ops, "POISON", True)                 # every output is 0xFF bytes until the kernel writes it
    for value in (-1, n - 1):
        label = torch.full((2, H, W), value, dtype=torch.int64)
        got = ops.label_onehot(label.to(dev), n).cpu()
        assert not bool(torch.isnan(got).any()) and torch.equal(got, one_hot_signal(label, n))
        assert float(got[:, value + 1].min()) == 1.0 and float(got.sum()) == 2 * H * W
    label, label_pos = random_labels(23, 2, n, H, W), random_labels(24, 2, n, H, W)
    a, b = ops.label_onehot(label.to(dev), n, label_pos.to(dev))
    assert torch.equal(a.cpu(), one_hot_signal(label, n)) and torch.equal(b.cpu(), one_hot_signal(label_pos, n))
    # a label outside the range under check=False: an all-zero pixel (the caller's contract), everything else as before
    broken = label.clone()
    broken[0, 1, 2], broken[1, 0, 0] = n, -2
    got = ops.label_onehot(broken.to(dev), n, check=False).cpu()
    assert torch.equal(got, ops.label_onehot(broken, n, check=False))
    assert float(got[0, :, 1, 2].sum()) == 0.0 and float(got[1, :, 0, 0].sum()) == 0.0
    with pytest.raises(ValueError, match=r"holds the value -2\b"):            # (the checked route names the lowest offender first)
        ops.label_onehot(broken.to(dev), n)


# ---- dg_fps_coords_large ----------------------------------------------------------------------------------------------------------
def _depth(seed, B, H, W):
    return torch.randint(0, 256, (B, 1, H, W), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("grid,depth_hw", [((28, 28), (56, 56)), ((64, 64), (64, 64))])
def test_fps_large_equals_fps_coords(grid, depth_hw, dev):
    """On a grid both entries accept: coordinates and selection order equal bit for bit, single launch and pair launch."""
    from depthg_amd import ops
    d, dp = _depth(31, 2, *depth_hw).to(dev), _depth(32, 2, *depth_hw).to(dev)
    want, want_inds = ops.fps_coords(d, grid, 11, return_inds=True)
    got, got_inds = ops.fps_coords_large(d, grid, 11, return_inds=True)
    assert torch.equal(got_inds, want_inds) and torch.equal(got, want)
    assert torch.equal(ops.fps_coords_large_pair(d, dp, grid, 11), ops.fps_coords_pair(d, dp, grid, 11))


def _flat(H, W):
    return torch.full((1, 1, H, W), 3.0)


def _far(H, W):
    d = torch.ones(1, 1, H, W)
    d[0, 0, H // 3, W - 2] = 200.0
    return d


FPS_ORACLE_CASES = {                                        # name -> (depth, grid)
    "65x64": (_depth(41, 2, 65, 64), (65, 64)),             # the first grid above the old limit
    "72x72_pooled": (_depth(42, 1, 144, 144), (72, 72)),    # through the pooling pre-pass
    "52x100": (_depth(43, 1, 52, 100), (52, 100)),
    "224x224": (_depth(44, 1, 224, 224), (224, 224)),       # the labels' resolution: 98 points per thread
    "256x256": (_depth(45, 1, 256, 256), (256, 256)),       # the limit: the depths are read again in every round
    "flat_80x80": (_flat(80, 80), (80, 80)),                # all distances tie: first arg-max
    "far_pixel_70x90": (_far(70, 90), (70, 90)),
}


@pytest.mark.parametrize("name", list(FPS_ORACLE_CASES))
def test_fps_large_equals_oracle(name, dev):
    from depthg_amd import ops
    from oracle import depthg_oracle as O
    depth, grid = FPS_ORACLE_CASES[name]
    want, want_inds = O.farthest_point_sampling_depth(grid, depth, 11, return_inds=True)
    got, got_inds = ops.fps_coords_large(depth.to(dev), grid, 11, return_inds=True)
    assert np.array_equal(got_inds.cpu().numpy(), np.asarray(want_inds))
    assert np.array_equal(got.cpu().numpy(), (want * 2 - 1).numpy())


# ---- the loss on one-hot signals ---------------------------------------------------------------------------------------------------
TRUE_LABEL_CASES = ["32x32_k4_fps_depth", "32x32_k28_none_depth", "32x32_k4_none_nodepth_nozc", "32x32_k28_fps_nodepth",
                    "64x72_k4_none_depth_nozc", "64x72_k28_fps_depth", "64x72_k4_fps_nodepth_nozc", "64x72_k28_none_nodepth"]


def _relclose(got, want, rtol, atol, what):
    got, want = float(got), float(want)
    assert abs(got - want) <= rtol * abs(want) + atol, f"{what}: got {got:.9e} want {want:.9e} rel {abs(got-want)/abs(want):.2e}"


@pytest.mark.parametrize("case", TRUE_LABEL_CASES)
def test_loss_on_onehot_signals_against_the_reference(case, dev):
    """The bounds of tests/test_gpu_parity.py::test_golden_forward_backward, unchanged."""
    from depthg_amd import ContrastiveCorrelationLoss, ops
    from oracle import depthg_oracle as O
    fx = load_golden(f"true_labels_{case}.npz")
    cfg = cfg_from_fixture(fx)
    T = lambda a: torch.from_numpy(a).to(dev)
    n_classes = int(fx["n_classes"])
    signal, signal_pos = ops.label_onehot(T(fx["label"]).long(), n_classes, T(fx["label_pos"]).long())
    loss = ContrastiveCorrelationLoss(cfg)
    if cfg.depth_sampling == "fps":
        # the coordinates the module draws on this signal (above 4096 positions: the large sampler) are the reference's
        c1, c2, shared = loss._draw_coords(signal, signal_pos, None, None, T(fx["depth"]), T(fx["depth_pos"]), same_maps=False)
        assert not shared and np.array_equal(c1.cpu().numpy(), fx["coords1"]) and np.array_equal(c2.cpu().numpy(), fx["coords2"])
    code, code_pos = T(fx["code"]).requires_grad_(True), T(fx["code_pos"]).requires_grad_(True)
    out = loss.forward_with(signal, signal_pos, code, code_pos, T(fx["depth"]), T(fx["coords1"]), T(fx["coords2"]), T(fx["perms"]))
    total = O.total_loss(cfg, out)
    total.backward()
    torch.cuda.synchronize()
    RT, AT = 1e-3, 1e-5
    _relclose(out[0], fx["pos_intra_loss"], RT, AT, "pos_intra_loss")
    _relclose(out[2], fx["pos_inter_loss"], RT, AT, "pos_inter_loss")
    _relclose(out[4].mean(), fx["neg_inter_loss_mean"], RT, AT, "neg_inter_loss.mean")
    _relclose(out[1].mean(), fx["pos_intra_cd_mean"], RT, 1e-5, "pos_intra_cd.mean")
    _relclose(out[3].mean(), fx["pos_inter_cd_mean"], RT, 1e-5, "pos_inter_cd.mean")
    _relclose(out[5].mean(), fx["neg_inter_cd_mean"], RT, 1e-5, "neg_inter_cd.mean")
    if cfg.depth_feat_correlation_loss:
        _relclose(out[6], fx["depth_feat_loss"], RT, AT, "depth_feat_loss")
        _relclose(out[7].mean(), fx["depth_feat_cd_mean"], 1e-6, 1e-7, "dd mean")
    _relclose(total, fx["total"], RT, AT, "total")
    sub = int(fx["sub"])
    pick = lambda t: t.detach().reshape(-1)[::sub].cpu().numpy()
    assert np.abs(pick(out[1]) - fx["pos_intra_cd"]).max() < 1e-3
    assert np.abs(pick(out[3]) - fx["pos_inter_cd"]).max() < 1e-3
    assert np.abs(pick(out[5]) - fx["neg_inter_cd"]).max() < 1e-3
    assert np.abs(pick(out[4]) - fx["neg_inter_loss"]).max() < 4e-3
    if cfg.depth_feat_correlation_loss:
        assert np.array_equal(pick(out[7]), fx["depth_feat_cd"])      # dd in {0,1}: exact
    for got, want, name in ((code.grad, fx["grad_code"], "grad_code"), (code_pos.grad, fx["grad_code_pos"], "grad_code_pos")):
        got, want = got.cpu().numpy().astype(np.float64), want.astype(np.float64)
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        cos = (got * want).sum() / (np.linalg.norm(got) * np.linalg.norm(want))
        tol = 3e-3 if not cfg.zero_clamp else 8e-3
        assert rel < tol and cos > 0.9995, f"{name}: rel-l2 {rel:.3e} cos {cos:.6f}"


# ---- one training step -------------------------------------------------------------------------------------------------------------
def _one_step(dev, **over):
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(3)
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(dim=16, feature_samples=4, neg_samples=2, res=32, **over)).to(dev).train()
    g = torch.Generator().manual_seed(1)
    batch = {"img": torch.randn(2, 3, 32, 32, generator=g), "img_pos": torch.randn(2, 3, 32, 32, generator=g),
             "label": torch.randint(-1, 5, (2, 32, 32), generator=g), "label_pos": torch.randint(-1, 5, (2, 32, 32), generator=g),
             "depth": torch.randint(1, 256, (2, 1, 32, 32), generator=g).float(),
             "depth_pos": torch.randint(1, 256, (2, 1, 32, 32), generator=g).float()}
    batch = {k: v.to(dev) for k, v in batch.items()}
    torch.manual_seed(7)
    loss, logs = seg.training_step(batch, 0)
    torch.cuda.synchronize()
    return loss, logs, [p.detach().clone() for p in seg.all_reduced_parameters()]


def test_training_step_with_true_labels(dev, monkeypatch):
    from depthg_amd import ops
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    loss, logs, params = _one_step(dev, use_true_labels=True)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v).all()) for v in logs.values())
    # the twin: the same model and draws, its loss call handed the torch-built one-hot maps
    calls = []

    def torch_chain(label, n_classes, label_pos, check=True):
        calls.append(check)
        return one_hot_signal(label, n_classes), one_hot_signal(label_pos, n_classes)

    with monkeypatch.context() as m:
        m.setattr(ops, "label_onehot", torch_chain)
        loss_t, logs_t, params_t = _one_step(dev, use_true_labels=True)
    assert calls == [True]
    assert torch.equal(loss, loss_t) and set(logs) == set(logs_t) and all(torch.equal(logs[k], logs_t[k]) for k in logs)
    assert len(params) == len(params_t) and all(torch.equal(a, b) for a, b in zip(params, params_t))
    # the switch is read: the unsupervised step of the same model gives another loss
    loss_u, logs_u, _ = _one_step(dev, use_true_labels=False)
    assert set(logs_u) == set(logs) and not torch.equal(loss, loss_u)
    assert not torch.equal(logs["loss/pos_intra"], logs_u["loss/pos_intra"])
