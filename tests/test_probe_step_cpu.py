"""CPU-side checks of the fused probe step (cfg.dg_fused_probes; head.fused_probe_losses over dg_probe_step_forward / _backward): the
exports, the flag and where it is read, the torch route CPU tensors take against the float64 restatement (tests/probe_step_reference.py),
the refusals, the margin of every case the GPU tests use, and that the step's plan did not grow."""
import re
from types import SimpleNamespace

import pytest
import torch

import probe_step_reference as R
from conftest import ROOT


def test_the_three_exports_and_their_argument_counts():
    from depthg_amd import _lib
    lib = _lib.load()
    want = {"dg_probe_step_workspace_bytes": 8, "dg_probe_step_forward": 17, "dg_probe_step_backward": 16}
    header = open(ROOT + "/include/depthg_corr.h").read()
    for name, count in want.items():
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert len(_lib.SIGNATURES[name][1]) == count
        proto = re.search(name + r"\s*\(([^()]*)\)\s*;", header)
        assert proto and len(proto.group(1).split(",")) == count
    assert "src/train_segmentation.py:421-444" in header and "src/modules.py:664-675" in header
    # served, and refused with the reason in front of any launch: no GPU is needed to ask
    assert lib.dg_probe_step_workspace_bytes(32, 70, 27, 27, 28, 28, 224, 224) > 0
    assert lib.dg_probe_step_workspace_bytes(1, 128, 64, 64, 56, 56, 1, 1) > 0
    for bad, why in (((2, 129, 27, 27, 4, 4, 8, 8), "D <= 128"), ((2, 70, 65, 27, 4, 4, 8, 8), "n_lin <= 64"),
                     ((2, 70, 27, 65, 4, 4, 8, 8), "n_clu <= 64"), ((2, 70, 64, 27, 4, 65, 8, 8), "n_lin * w <= 4096")):
        assert lib.dg_probe_step_workspace_bytes(*bad) == 0
        assert why in lib.dg_last_error().decode()
        assert lib.dg_probe_step_forward(None, None, None, None, None, *bad, None, None, 0, None) == -2       # DG_ERR_UNSUPPORTED
    assert lib.dg_probe_step_forward(None, None, None, None, None, 2, 8, 3, 5, 4, 4, 8, 8, None, None, 0, None) == -1   # null pointers


def test_the_flag_is_off_by_default_and_read_at_construction():
    from depthg_amd import segmenter as S
    assert S.default_segmenter_cfg().dg_fused_probes is False
    from depthg_amd import head
    assert S.fused_probe_losses is head.fused_probe_losses            # re-exported where probe_cross_entropy is
    off = S.UnsupervisedSegmenter(5, S.default_segmenter_cfg(res=16))
    assert off.fused_probes is False
    bare = S.default_segmenter_cfg(res=16)
    del bare.dg_fused_probes
    assert S.UnsupervisedSegmenter(5, bare).fused_probes is False
    on = S.UnsupervisedSegmenter(5, S.default_segmenter_cfg(res=16, dg_fused_probes=True))
    assert on.fused_probes is True
    on.cfg.dg_fused_probes = False                    # (read once: a later change of cfg does not change the route)
    assert on.fused_probes is True


def _probe_inputs(shape="tiny"):
    code, label, weight, bias, clusters = R.operands(shape)
    return code, label, weight, bias, clusters


def test_a_step_without_the_flag_makes_no_call(monkeypatch):
    from depthg_amd import segmenter as S
    code, label, *_ = _probe_inputs()
    calls = []
    monkeypatch.setattr(S, "fused_probe_losses", lambda *a: calls.append(a) or (torch.zeros(()), torch.zeros(())))
    monkeypatch.setattr(S, "probe_cross_entropy", lambda logits, lab: logits.sum() * 0)
    m = S.UnsupervisedSegmenter(3, S.default_segmenter_cfg(res=16, dim=8))
    monkeypatch.setattr(type(m.cluster_probe), "forward", lambda self, x, alpha: (x.sum() * 0, None))
    logs = {}
    m._probe_terms(code, label, 0, logs)
    assert not calls and set(logs) == {"loss/linear", "loss/cluster", "loss/total"}


def test_probe_terms_with_the_flag_logs_the_same_keys_and_trains_the_probes():
    from depthg_amd import segmenter as S
    code, label, *_ = _probe_inputs()
    torch.manual_seed(0)
    m = S.UnsupervisedSegmenter(3, S.default_segmenter_cfg(res=16, dim=8, extra_clusters=2, dg_fused_probes=True))
    logs = {}
    attached = code.clone().requires_grad_(True)       # the step's code carries a graph: _probe_terms detaches it
    loss = m._probe_terms(attached * 1.0, label, 0, logs)
    assert set(logs) == {"loss/linear", "loss/cluster", "loss/total"}
    assert float(logs["loss/total"]) == pytest.approx(float(logs["loss/linear"]) + float(logs["loss/cluster"]), rel=1e-6)
    loss.backward()
    assert attached.grad is None
    t = R.chain(code, label, m.linear_probe.weight.detach(), m.linear_probe.bias.detach(), m.cluster_probe.clusters.detach())
    assert float(logs["loss/linear"]) == pytest.approx(t["linear_loss"], rel=1e-5)
    assert float(logs["loss/cluster"]) == pytest.approx(t["cluster_loss"], rel=1e-5)
    for p, k in ((m.linear_probe.weight, "d_weight"), (m.linear_probe.bias, "d_bias"), (m.cluster_probe.clusters, "d_clusters")):
        assert p.grad is not None and float((p.grad.double().reshape(t[k].shape) - t[k]).norm() / t[k].norm()) < 1e-5, k


@pytest.mark.parametrize("shape", ["tiny", "ragged", "ratios", "limits"])
@pytest.mark.parametrize("upstream", R.UPSTREAM)
def test_the_cpu_route_agrees_with_the_restatement(shape, upstream):
    from depthg_amd.head import fused_probe_losses
    got, t = R.run(fused_probe_losses, R.operands(shape), upstream, "cpu"), R.truth(shape, upstream)
    f = R.figures(got, t)
    assert f["linear_loss"] <= 1e-5 * abs(t["linear_loss"]) and f["cluster_loss"] <= 1e-5 * abs(t["cluster_loss"]), f
    assert all(f[k] <= 1e-5 for k in R.GRADS), f
    # the yardstick is the same chain
    y = R.figures(R.run(R.torch_chain, R.operands(shape), upstream, "cpu"), t)
    assert all(y[k] <= 1e-5 for k in R.GRADS), y


def test_the_restatements_resize_is_interpolate():
    g = torch.Generator().manual_seed(1)
    for (h, w), (H, W) in (((4, 4), (8, 8)), ((7, 7), (20, 33)), ((3, 3), (5, 4)), ((5, 7), (3, 2)), ((1, 1), (4, 5))):
        x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64)
        want = torch.nn.functional.interpolate(x, (H, W), mode="bilinear", align_corners=False)
        got = torch.einsum("Yy,bnyx,Xx->bnYX", R.resize_matrix(H, h), x, R.resize_matrix(W, w))
        assert float((got - want).abs().max()) < 1e-12


def test_every_gpu_case_keeps_the_margin_and_the_label_patterns():
    for shape, (B, D, n, m, hw, HW) in R.SHAPES.items():
        code, label, weight, bias, clusters = R.operands(shape)
        assert float(R.top_two_gap(code, clusters).min()) >= R.GAP, shape
        assert tuple(code.shape) == (B, D) + hw and tuple(label.shape) == (B,) + HW and tuple(clusters.shape) == (m, D)
        assert bool((label == -1).any()) and bool((label >= n).any()) and bool((label[0, HW[0] // 2] == -1).all())
        assert bool(((label >= 0) & (label < n)).any())
        if B > 1:
            assert not bool(((label[B - 1] >= 0) & (label[B - 1] < n)).any())
        # the float32 arg-max is the float64 one
        inner = torch.einsum("bchw,nc->bnhw", torch.nn.functional.normalize(code, dim=1), torch.nn.functional.normalize(clusters, dim=1))
        assert torch.equal(inner.argmax(1), R.truth(shape)["arg"])
    with pytest.raises(AssertionError, match="closer than GAP"):
        # two equal centres: no draw of the code separates them
        gen = torch.Generator().manual_seed(0)
        real_randn = torch.randn
        try:
            torch.randn = lambda *s, generator=None: torch.ones(*s) if len(s) == 2 else real_randn(*s, generator=generator)
            R.margin_inputs(1, 4, 3, (2, 2), gen)
        finally:
            torch.randn = real_randn


def test_refusals():
    from depthg_amd.head import fused_probe_losses
    code, label, weight, bias, clusters = _probe_inputs()
    with pytest.raises(RuntimeError, match="requires grad.*probe_cross_entropy"):
        fused_probe_losses(code.clone().requires_grad_(True), label, weight, bias, clusters)
    with pytest.raises(RuntimeError, match="D <= 128"):
        fused_probe_losses(torch.randn(1, 129, 2, 2), label[:1], torch.randn(3, 129, 1, 1), bias, torch.randn(5, 129))
    with pytest.raises(RuntimeError, match="n_lin <= 64"):
        fused_probe_losses(code, label, torch.randn(65, 8, 1, 1), torch.randn(65), clusters)
    with pytest.raises(RuntimeError, match="n_clu <= 64"):
        fused_probe_losses(code, label, weight, bias, torch.randn(65, 8))
    with pytest.raises(ValueError, match=r"label must be \(B, H, W\)"):
        fused_probe_losses(code, label[0], weight, bias, clusters)
    with pytest.raises(ValueError, match=r"label must be \(B, H, W\)"):
        fused_probe_losses(code, label[:, None].expand(-1, 2, -1, -1), weight, bias, clusters)
    with pytest.raises(ValueError, match="label holds 1 images, code 2"):
        fused_probe_losses(code, label[:1], weight, bias, clusters)
    with pytest.raises(ValueError, match="clusters must be"):
        fused_probe_losses(code, label, weight, bias, torch.randn(5, 9))
    # (B, 1, H, W) labels are the dataset's form
    a, b = fused_probe_losses(code, label[:, None], weight, bias, clusters), fused_probe_losses(code, label, weight, bias, clusters)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_step_plan_is_unchanged_and_the_recording_keys_the_attribute():
    from depthg_amd import graph_step, training
    assert len(training.StepPlan._fields) == 16 and "fused_probes" not in training.StepPlan._fields
    seen = []

    class Wrapper(graph_step.GraphedTrainStep):
        def __init__(self, flag):
            cfg = SimpleNamespace()
            self.model = SimpleNamespace(cfg=cfg, contrastive_corr_loss_fn=SimpleNamespace(cfg=cfg), training=True,
                                         net=SimpleNamespace(training=True), fused_probes=flag)
    assert Wrapper(True).capture_key() != Wrapper(False).capture_key()
    assert Wrapper(False).capture_key()[:-1] == Wrapper(True).capture_key()[:-1] and not seen


def test_the_train_command_has_the_flag():
    src = open(ROOT + "/depthg_amd/train.py").read()
    assert '"--fused-probes"' in src and 'overrides["dg_fused_probes"] = True' in src
