"""cfg.use_true_labels without a GPU: the CPU route of ops.label_onehot against F.one_hot, the refusals of the op, of the two C entries
(in front of any launch), of the loss's samplers, of the training step and of the recorded step, the exports, and that a default step
never reaches the new op."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_onehot_reference import ONEHOT_SHAPES, one_hot_signal, random_labels  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B,K,H,W", ONEHOT_SHAPES)
def test_cpu_route_is_the_reference_chain(B, K, H, W):
    from depthg_amd import ops
    label, label_pos = random_labels(11, B, K - 1, H, W), random_labels(12, B, K - 1, H, W)
    want, want_pos = one_hot_signal(label, K - 1), one_hot_signal(label_pos, K - 1)
    got = ops.label_onehot(label, K - 1)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, K, H, W) and torch.equal(got, want)
    a, b = ops.label_onehot(label, K - 1, label_pos)
    assert torch.equal(a, want) and torch.equal(b, want_pos)
    assert torch.equal(ops.label_onehot(label.unsqueeze(1), K - 1), want)              # (B,1,H,W)
    assert torch.equal(ops.label_onehot(label, K - 1, check=False), want)              # the unchecked route: the same map in range
    assert float(got.sum()) == B * H * W                                                # one channel per pixel


def test_unchecked_route_writes_zeros_for_a_label_outside_the_range():
    from depthg_amd import ops
    label = torch.tensor([[[0, 3, -2, 1]]])
    got = ops.label_onehot(label, 3, check=False)
    assert tuple(got.shape) == (1, 4, 1, 4)
    assert got[0, :, 0, 0].tolist() == [0, 1, 0, 0] and got[0, :, 0, 3].tolist() == [0, 0, 1, 0]
    assert float(got[0, :, 0, 1].sum()) == 0.0 and float(got[0, :, 0, 2].sum()) == 0.0


def test_label_onehot_refusals():
    from depthg_amd import ops
    label = random_labels(3, 2, 4, 6, 6)
    for bad in (4, -2, 999):
        broken = label.clone()
        broken[1, 2, 3] = bad
        with pytest.raises(ValueError, match=rf"holds the value {bad}\b"):
            ops.label_onehot(broken, 4)
        with pytest.raises(ValueError, match=r"`label_pos` holds the value"):
            ops.label_onehot(label, 4, broken)
    with pytest.raises(ValueError, match="int64"):
        ops.label_onehot(label.int(), 4)
    with pytest.raises(ValueError, match="int64"):
        ops.label_onehot(label.float(), 4)
    with pytest.raises(ValueError, match=r"\(B,H,W\) or \(B,1,H,W\)"):
        ops.label_onehot(label.view(2, 2, 3, 6), 4)
    with pytest.raises(ValueError, match="256"):
        ops.label_onehot(label, 256)
    with pytest.raises(ValueError, match="must match"):
        ops.label_onehot(label, 4, label[:1])


def test_exports_and_signatures():
    from depthg_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in ("dg_label_onehot", "dg_fps_coords_large", "dg_fps_large_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf"\b{name}\s*\(", header), name
    assert _lib.SIGNATURES["dg_fps_coords_large"] == _lib.SIGNATURES["dg_fps_coords"]          # the same parameters
    assert len(_lib.SIGNATURES["dg_label_onehot"][1]) == 8
    assert lib.dg_fps_large_workspace_bytes(2, 224, 224) >= 2 * 224 * 224 * 4
    m = re.search(r"#define\s+DG_VERSION\s+(\d+)\b", header)
    assert lib.dg_version() == _lib.DG_VERSION == int(m.group(1))
    for name in ("label_onehot", "fps_coords_large", "fps_coords_large_pair"):
        assert callable(getattr(ops, name))
    # src/train_segmentation.py:219-225 is cited where the entry is declared
    assert "src/train_segmentation.py:219-225" in header


def _err():
    from depthg_amd import _lib
    return _lib.load().dg_last_error().decode()


def test_c_entries_refuse_before_any_launch():
    """Null and misaligned pointers and the grid limits, on host memory: a launch would fault, a refusal returns."""
    from depthg_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = lambda off=0: ctypes.c_void_p(base + off)
    fps = lambda depth, pos, B, H, W, h, w, S, out, inds=None, ws=None, nws=0: \
        lib.dg_fps_coords_large(depth, pos, B, H, W, h, w, S, out, inds, ws, nws, None)
    assert fps(None, None, 1, 80, 80, 80, 80, 3, p()) < 0 and "null pointer" in _err()
    assert fps(p(), None, 1, 80, 80, 80, 80, 3, None) < 0 and "null pointer" in _err()
    assert fps(p(2), None, 1, 80, 80, 80, 80, 3, p()) < 0 and "aligned" in _err()
    assert fps(p(), None, 1, 80, 80, 80, 80, 3, p(1)) < 0 and "aligned" in _err()
    assert fps(p(), None, 1, 300, 300, 300, 300, 3, p()) < 0 and "dg_fps_coords_large" in _err() and "65536" in _err()
    assert fps(p(), None, 1, 2, 2, 2, 2, 3, p()) < 0 and "cannot sample 9 points from a 2x2 map" in _err()
    assert fps(p(), None, 1, 200, 200, 200, 200, 91, p()) < 0 and "8192" in _err()
    assert fps(p(), None, 1, 70, 70, 80, 80, 3, p()) < 0 and "dimensions" in _err()                    # depth smaller than the grid
    assert fps(p(), None, 1, 160, 160, 80, 80, 3, p()) < 0 and "workspace" in _err()                   # pooling without a workspace
    assert fps(p(), None, 1, 160, 160, 80, 80, 3, p(), None, p(), 64) < 0 and "workspace" in _err()
    assert fps(p(), None, 1, 2, 20000, 1, 20000, 3, p(), None, p(), 1 << 20) < 0 and "64 KB" in _err()  # the pre-pass's LDS condition
    assert fps(p(), None, 0, 80, 80, 80, 80, 3, p()) < 0
    # the existing entry keeps its limit
    assert lib.dg_fps_coords(p(), None, 1, 80, 80, 80, 80, 3, p(), None, None, 0, None) < 0 and "max 4096 pixels" in _err()
    oh = lambda label, pos, B, n, H, W, out: lib.dg_label_onehot(label, pos, B, n, H, W, out, None)
    assert oh(None, None, 1, 3, 4, 4, p()) < 0 and "null pointer" in _err()
    assert oh(p(), None, 1, 3, 4, 4, None) < 0 and "null pointer" in _err()
    assert oh(p(4), None, 1, 3, 4, 4, p()) < 0 and "8-byte" in _err()
    assert oh(p(), p(4), 1, 3, 4, 4, p()) < 0 and "8-byte" in _err()
    assert oh(p(), None, 1, 3, 4, 4, p(2)) < 0 and "4-byte" in _err()
    assert oh(p(), None, 1, 256, 4, 4, p()) < 0 and "256" in _err()
    assert oh(p(), p(), 40000, 3, 4, 4, p()) < 0 and "65535" in _err()
    assert oh(p(), None, 1, 3, 5000, 5000, p()) < 0 and "2^24" in _err()
    assert oh(p(), None, 0, 3, 4, 4, p()) < 0 and oh(p(), None, 1, -1, 4, 4, p()) < 0


def test_samplers_that_stay_at_4096_positions_name_the_way_out():
    from depthg_amd import ContrastiveCorrelationLoss
    from oracle import depthg_oracle as O
    sig = torch.zeros(1, 4, 72, 64)
    depth = torch.ones(1, 1, 72, 64)
    for over, what in ((dict(depth_sampling="simple"), "simple"), (dict(depth_sampling="fps_depth_feat", dg_fps_feats=True), "dg_fps_feats")):
        loss = ContrastiveCorrelationLoss(O.default_cfg(feature_samples=5, **over))
        with pytest.raises(ValueError, match="use_true_labels") as e:
            loss._draw_coords(sig, sig, None, None, depth, depth)
        assert what in str(e.value) and "depth_sampling = 'fps'" in str(e.value) and "'none'" in str(e.value) and "72x64" in str(e.value)


def _segmenter(**over):
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(0)
    return UnsupervisedSegmenter(5, default_segmenter_cfg(dim=16, feature_samples=5, neg_samples=2, res=32, **over)).train()


def _batch(with_pos=True):
    g = torch.Generator().manual_seed(1)
    batch = {"img": torch.randn(2, 3, 32, 32, generator=g), "img_pos": torch.randn(2, 3, 32, 32, generator=g),
             "label": torch.randint(-1, 5, (2, 32, 32), generator=g), "depth": torch.rand(2, 1, 32, 32, generator=g),
             "depth_pos": torch.rand(2, 1, 32, 32, generator=g)}
    if with_pos:
        batch["label_pos"] = torch.randint(-1, 5, (2, 32, 32), generator=g)
    return batch


def test_training_step_refusals_come_before_any_launch(monkeypatch):
    from depthg_amd.segmenter import UnsupervisedSegmenter
    seg = _segmenter(use_true_labels=True)
    # (a CPU model: the first launch of a step would raise "there is no CPU path" - the refusals below come in front of it)
    monkeypatch.setattr(seg, "_anchor_pass", lambda *a, **k: pytest.fail("the featurizer pass started"))
    with pytest.raises(KeyError, match="label_pos"):
        seg.training_step(_batch(with_pos=False))
    cfg = SimpleNamespace(use_true_labels=True, use_depth_only_intra=True)
    with pytest.raises(ValueError, match="use_depth_only_intra"):
        UnsupervisedSegmenter._refuse_true_labels_combinations(cfg, _batch())
    seg.cfg.use_depth_only_intra = True
    with pytest.raises(ValueError, match="use_true_labels cannot be combined with cfg.use_depth_only_intra"):
        seg.training_step(_batch())


def test_graphed_step_refuses_the_key_and_keeps_its_capture_key():
    from depthg_amd import graph_step
    cfg = SimpleNamespace(dg_feature_cache="float32", dg_graph_safe=True, dg_fused_adam=True, use_true_labels=True)
    with pytest.raises(ValueError, match="use_true_labels"):
        graph_step.refuse(cfg, object(), object())
    cfg.use_true_labels = False
    graph_step.refuse(cfg, object(), object())
    assert "use_true_labels" not in graph_step.CAPTURE_KEY


@pytest.mark.parametrize("over", [{}, {"use_true_labels": False}])
def test_default_step_never_reaches_the_new_op(over, monkeypatch):
    """use_true_labels absent or False: the correspondence stage hands the loss the featurizer's maps and calls nothing new."""
    from depthg_amd import ops
    seg = _segmenter(**over)
    if not over:
        del seg.cfg.use_true_labels           # the key absent, not merely False
    calls = []
    for name in ("label_onehot", "fps_coords_large", "fps_coords_large_pair"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    seen = []

    class Reached(Exception):
        pass

    def loss_call(*a, **k):
        seen.append(a)
        raise Reached

    monkeypatch.setattr(seg.contrastive_corr_loss_fn, "forward", loss_call)
    feats, code = torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 4, 4)
    p = SimpleNamespace(feats=feats, feats_pos=feats + 1, code=code, code_pos=code, image_feat=None, image_feat_pos=None)
    plan = SimpleNamespace(use_salience=False, depth_term=False, depth_only_intra=False, histograms=False, lhp=False)
    with pytest.raises(Reached):
        seg._correspondence_term(plan, _batch(), p, (None, None), (None, None))
    assert not calls and seen[0][0] is feats and seen[0][1] is p.feats_pos
    # ... and with the key set the stage asks the op for both maps at once and passes them on
    seg.cfg.use_true_labels = True
    signal = (torch.ones(1), torch.zeros(1))
    monkeypatch.setattr(ops, "label_onehot", lambda label, n, label_pos, check: calls.append((n, check)) or signal)
    seen.clear()
    with pytest.raises(Reached):
        seg._correspondence_term(plan, _batch(), p, (None, None), (None, None))
    assert calls == [(5, True)] and seen[0][0] is signal[0] and seen[0][1] is signal[1]
    seg.cfg.dg_graph_safe = True
    with pytest.raises(Reached):
        seg._correspondence_term(plan, _batch(), p, (None, None), (None, None))
    assert calls[-1] == (5, False)
