"""The correlation loss on signals above 16384 positions (cfg.use_true_labels at the labels' resolution; Sampler::Direct,
k_sample_direct): against the reference's fixtures (tests/golden/large_signal_*.npz, scripts/make_large_signal_fixtures.py) and, at
the limit, against the oracle on the CPU - within the bounds of tests/test_gpu_true_labels.py::
test_loss_on_onehot_signals_against_the_reference, unchanged - and one training step on 136 x 128 labels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import cfg_from_fixture, load_golden  # noqa: E402
from label_onehot_reference import one_hot_signal  # noqa: E402

pytestmark = pytest.mark.gpu

SUB = 37
RT, AT = 1e-3, 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def _relclose(got, want, rtol, atol, what):
    got, want = float(got), float(want)
    assert abs(got - want) <= rtol * abs(want) + atol, f"{what}: got {got:.9e} want {want:.9e} rel {abs(got-want)/abs(want):.2e}"


def _check(cfg, out, total, grads, want):
    """`want`: the fixture's keys (means, every SUB-th element of the un-reduced tensors, total, gradients)."""
    _relclose(out[0], want["pos_intra_loss"], RT, AT, "pos_intra_loss")
    _relclose(out[2], want["pos_inter_loss"], RT, AT, "pos_inter_loss")
    _relclose(out[4].mean(), want["neg_inter_loss_mean"], RT, AT, "neg_inter_loss.mean")
    _relclose(out[1].mean(), want["pos_intra_cd_mean"], RT, 1e-5, "pos_intra_cd.mean")
    _relclose(out[3].mean(), want["pos_inter_cd_mean"], RT, 1e-5, "pos_inter_cd.mean")
    _relclose(out[5].mean(), want["neg_inter_cd_mean"], RT, 1e-5, "neg_inter_cd.mean")
    if cfg.depth_feat_correlation_loss:
        _relclose(out[6], want["depth_feat_loss"], RT, AT, "depth_feat_loss")
        _relclose(out[7].mean(), want["depth_feat_cd_mean"], 1e-6, 1e-7, "dd mean")
    _relclose(total, want["total"], RT, AT, "total")
    pick = lambda t: t.detach().reshape(-1)[::SUB].cpu().numpy()
    assert np.abs(pick(out[1]) - want["pos_intra_cd"]).max() < 1e-3
    assert np.abs(pick(out[3]) - want["pos_inter_cd"]).max() < 1e-3
    assert np.abs(pick(out[5]) - want["neg_inter_cd"]).max() < 1e-3
    assert np.abs(pick(out[4]) - want["neg_inter_loss"]).max() < 4e-3
    if cfg.depth_feat_correlation_loss:
        assert np.array_equal(pick(out[7]), want["depth_feat_cd"])      # dd in {0,1}: exact
    for got, name in zip(grads, ("grad_code", "grad_code_pos")):
        got, ref = got.cpu().numpy().astype(np.float64), want[name].astype(np.float64)
        rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        cos = (got * ref).sum() / (np.linalg.norm(got) * np.linalg.norm(ref))
        tol = 3e-3 if not cfg.zero_clamp else 8e-3
        assert rel < tol and cos > 0.9995, f"{name}: rel-l2 {rel:.3e} cos {cos:.6f}"


# ---- the loss against the reference ------------------------------------------------------------------------------------------------
LARGE_SIGNAL_CASES = ["136x124_k28_fps_depth", "136x124_k4_none_nodepth_nozc", "256x256_k28_none_depth", "136x124_k4_fps_depth_S14"]


@pytest.mark.parametrize("case", LARGE_SIGNAL_CASES)
def test_loss_on_large_signals_against_the_reference(case, dev):
    from depthg_amd import ContrastiveCorrelationLoss, ops
    from oracle import depthg_oracle as O
    fx = load_golden(f"large_signal_{case}.npz")
    cfg = cfg_from_fixture(fx)
    T = lambda a: torch.from_numpy(a).to(dev)
    n_classes = int(fx["n_classes"])
    signal, signal_pos = ops.label_onehot(T(fx["label"]).long(), n_classes, T(fx["label_pos"]).long())
    assert signal.shape[-2] * signal.shape[-1] > 16384
    loss = ContrastiveCorrelationLoss(cfg)
    if cfg.depth_sampling == "fps":
        c1, c2, shared = loss._draw_coords(signal, signal_pos, None, None, T(fx["depth"]), T(fx["depth_pos"]), same_maps=False)
        assert not shared and np.array_equal(c1.cpu().numpy(), fx["coords1"]) and np.array_equal(c2.cpu().numpy(), fx["coords2"])
    code, code_pos = T(fx["code"]).requires_grad_(True), T(fx["code_pos"]).requires_grad_(True)
    out = loss.forward_with(signal, signal_pos, code, code_pos, T(fx["depth"]), T(fx["coords1"]), T(fx["coords2"]), T(fx["perms"]))
    # S = 14 takes the blob path behind k_gather_norm, the others the fused small-grid kernel
    assert (ops.corr_main_kernel_name(loss.last_call[0]) == "k_corr_small") == (cfg.feature_samples <= 12)
    total = O.total_loss(cfg, out)
    total.backward()
    torch.cuda.synchronize()
    _check(cfg, out, total, (code.grad, code_pos.grad), fx)


def test_loss_at_the_limit_against_the_oracle(dev):
    """Beyond the fixtures: a non-square 181 x 362 map (65522 positions, just under the limit), given coordinates - some beyond the
    border - and batch maps, held to the oracle on the CPU at the fixtures' bounds."""
    from depthg_amd import ContrastiveCorrelationLoss
    from oracle import depthg_oracle as O
    B, K, D, H, W, S, N = 2, 4, 24, 181, 362, 11, 3
    g = torch.Generator().manual_seed(77)
    label, label_pos = (torch.randint(-1, K - 1, (B, H // 4 + 1, W // 4 + 1), generator=g).repeat_interleave(4, 1)
                        .repeat_interleave(4, 2)[:, :H, :W].contiguous() for _ in range(2))
    signal, signal_pos = one_hot_signal(label, K - 1), one_hot_signal(label_pos, K - 1)
    code, code_pos = torch.randn(B, D, 8, 8, generator=g), torch.randn(B, D, 8, 8, generator=g)
    depth = torch.randint(0, 256, (B, 1, H, W), generator=g).float()
    coords1, coords2 = (torch.rand(B, S, S, 2, generator=g) * 2.1 - 1.05 for _ in range(2))
    perms = torch.stack([torch.tensor([1, 0]), torch.tensor([1, 0]), torch.tensor([0, 1])])
    cfg = O.default_cfg(feature_samples=S, neg_samples=N)
    c, cp = code.clone().requires_grad_(True), code_pos.clone().requires_grad_(True)
    ref = O.forward(cfg, signal, signal_pos, c, cp, depth=depth, coords1=coords1, coords2=coords2, perms=list(perms))
    ref_total = O.total_loss(cfg, ref)
    ref_total.backward()
    pick = lambda t: t.detach().reshape(-1)[::SUB].numpy()
    want = dict(pos_intra_loss=ref[0].item(), pos_inter_loss=ref[2].item(), neg_inter_loss_mean=ref[4].mean().item(),
                pos_intra_cd_mean=ref[1].mean().item(), pos_inter_cd_mean=ref[3].mean().item(), neg_inter_cd_mean=ref[5].mean().item(),
                depth_feat_loss=ref[6].item(), depth_feat_cd_mean=ref[7].mean().item(), total=ref_total.item(),
                pos_intra_cd=pick(ref[1]), pos_inter_cd=pick(ref[3]), neg_inter_cd=pick(ref[5]), neg_inter_loss=pick(ref[4]),
                depth_feat_cd=pick(ref[7]), grad_code=c.grad.numpy(), grad_code_pos=cp.grad.numpy())
    code_d, code_pos_d = code.to(dev).requires_grad_(True), code_pos.to(dev).requires_grad_(True)
    loss = ContrastiveCorrelationLoss(cfg)
    out = loss.forward_with(signal.to(dev), signal_pos.to(dev), code_d, code_pos_d, depth.to(dev), coords1.to(dev), coords2.to(dev), perms.to(dev))
    total = O.total_loss(cfg, out)
    total.backward()
    torch.cuda.synchronize()
    _check(cfg, out, total, (code_d.grad, code_pos_d.grad), want)


# ---- one training step -------------------------------------------------------------------------------------------------------------
H_IMG, W_IMG = 136, 128            # 17408 label positions over 17 x 16 code maps


def _one_step(dev, sampling, record=None):
    from depthg_amd.loss import ContrastiveCorrelationLoss
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(3)
    cfg = default_segmenter_cfg(dim=16, feature_samples=4, neg_samples=2, res=H_IMG, use_true_labels=True, depth_sampling=sampling)
    seg = UnsupervisedSegmenter(5, cfg).to(dev).train()
    g = torch.Generator().manual_seed(1)
    shape = (2, H_IMG, W_IMG)
    batch = {"img": torch.randn(2, 3, H_IMG, W_IMG, generator=g), "img_pos": torch.randn(2, 3, H_IMG, W_IMG, generator=g),
             "label": torch.randint(-1, 5, shape, generator=g), "label_pos": torch.randint(-1, 5, shape, generator=g),
             "depth": torch.randint(1, 256, (2, 1, H_IMG, W_IMG), generator=g).float(),
             "depth_pos": torch.randint(1, 256, (2, 1, H_IMG, W_IMG), generator=g).float()}
    batch = {k: v.to(dev) for k, v in batch.items()}
    torch.manual_seed(7)
    loss_fn = seg.contrastive_corr_loss_fn
    inner = ContrastiveCorrelationLoss.forward_with

    def recording(self, *args, **kw):
        out = inner(self, *args, **kw)
        if record is not None:
            record.append(([a.detach().cpu() if isinstance(a, torch.Tensor) else a for a in args[:7]], self.last_call[1].cpu()))
        return out

    loss_fn.forward_with = recording.__get__(loss_fn)
    loss, logs = seg.training_step(batch, 0)
    torch.cuda.synchronize()
    return seg.cfg, loss, logs


@pytest.mark.parametrize("sampling", ["fps", "none"])
def test_training_step_on_a_large_label_signal(sampling, dev, monkeypatch):
    from depthg_amd import ops
    from oracle import depthg_oracle as O
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    calls = []
    cfg, loss, logs = _one_step(dev, sampling, calls)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v).all()) for v in logs.values())
    # the three correspondence logs: the oracle on the arguments the loss call received and the batch maps it drew
    assert len(calls) == 1
    (signal, signal_pos, code, code_pos, depth, coords1, coords2), perms = calls[0]
    assert tuple(signal.shape) == (2, 6, H_IMG, W_IMG) and tuple(code.shape) == (2, 16, H_IMG // 8, W_IMG // 8) and tuple(perms.shape) == (2, 2)
    ref = O.forward(cfg, signal, signal_pos, code, code_pos, depth=depth, coords1=coords1, coords2=coords2, perms=list(perms))
    _relclose(logs["loss/pos_intra"], ref[0], RT, AT, "loss/pos_intra")
    _relclose(logs["loss/pos_inter"], ref[2], RT, AT, "loss/pos_inter")
    _relclose(logs["loss/neg_inter"], ref[4].mean(), RT, AT, "loss/neg_inter")
    # the twin: the same model and draws, its loss call handed the torch-built one-hot maps
    with monkeypatch.context() as m:
        m.setattr(ops, "label_onehot", lambda label, n_classes, label_pos, check=True: (one_hot_signal(label, n_classes),
                                                                                        one_hot_signal(label_pos, n_classes)))
        _, loss_t, logs_t = _one_step(dev, sampling)
    assert torch.equal(loss, loss_t) and set(logs) == set(logs_t) and all(torch.equal(logs[k], logs_t[k]) for k in logs)
