"""GraphedTrainStep on the GPU against the parent route - DeviceEpoch.batch feeding training_step eagerly - on 12 images, B = 4, 5 x 5
feature grids, a float32 feature cache and deterministic torch algorithms (as tests/test_gpu_feature_cache.py).  Every case runs the
eager route twice first (A, A') and holds the graphed run G to A bit for bit wherever A' repeats A, else to the pair's own distance."""
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

import data_folders as DF
from conftest import ROOT
from epoch_draw_reference import case
from sample_cache_cases import CROPPED, MemorySet, make_samples

pytestmark = pytest.mark.gpu

N_IMAGES, B, NUM_NEIGHBORS, RES, STEPS = 12, 4, 3, 40, 4
SOURCE_SIZES = [(40, 40), (44, 48), (52, 40), (40, 56)] * 3                     # (width, height): a centre crop of 40 x 40 from each


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _cfg(kind, **over):
    from depthg_amd.segmenter import default_segmenter_cfg
    if kind == "dino":          # the two-block ViT (head dimension 64), 40 x 40 images: a 5 x 5 feature grid
        base = dict(model_type="vit_small", dino_patch_size=8, dg_dino_backbone=True, feature_samples=5,
                    dg_dino_vit_kwargs=dict(img_size=[32], embed_dim=128, depth=2, num_heads=2))
    else:                       # the stand-in backbone at 40 x 40: the same 5 x 5 grid, 384 channels
        base = dict(dim=70, feature_samples=5)
    return default_segmenter_cfg(**{**base, "dg_feature_cache": "float32", "dg_graph_safe": True, "dg_fused_adam": True, "dg_graph_step": True,
                                    "hist_freq": None, **over})


def _segmenter(kind, dev, **over):
    from depthg_amd.segmenter import UnsupervisedSegmenter
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)            # (the ViT keeps its seeded random weights)
        seg = UnsupervisedSegmenter(5, _cfg(kind, **over)).to(dev)
    seg.train()
    return seg


_CACHES = {}


def _caches(kind, dev):
    """(sample cache, feature cache, table) of the 12 images, built once per backbone with the seeded model every run rebuilds."""
    if kind not in _CACHES:
        from depthg_amd import data
        was = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            ds = MemorySet(make_samples(SOURCE_SIZES, labels=True, depth="bytes", n_label=6), **CROPPED)
            seg = _segmenter(kind, dev)
            samples = data.build_sample_cache(ds, seg.cfg, RES, "center", True, dev, 0, image_set="train")
            feats = data.build_feature_cache(seg.net, ds, seg.cfg, RES, "center", dtype=torch.float32, device=dev, batch_size=N_IMAGES)
        finally:
            torch.backends.cudnn.deterministic = was
        _CACHES[kind] = (samples, feats, case(N_IMAGES, 6)[1])
    return _CACHES[kind]


def _run(kind, dev, graphed, over, monkeypatch, strict=True):
    """STEPS steps (3 an epoch: the fourth opens a second one) of a freshly seeded model, optimiser and epoch.  -> (per step (loss, logs),
    the stepped parameters after the last, the GraphedTrainStep or None)."""
    from depthg_amd.epoch import DeviceEpoch
    from depthg_amd.graph_step import GraphedTrainStep, make_capturable
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    samples, feats, nns = _caches(kind, dev)
    seg = _segmenter(kind, dev, **over)
    torch.manual_seed(7)
    ep = DeviceEpoch(nns, B, NUM_NEIGHBORS, dev, shuffle=True, generator=torch.Generator().manual_seed(5))
    assert ep.steps_per_epoch == 3
    wrapper = None
    if graphed:
        wrapper = GraphedTrainStep(seg, ep, samples, feats, strict=strict)
        step = wrapper.step
    else:
        make_capturable(seg)
        step = lambda: seg.training_step(ep.batch(samples, feats))
    outs, flags = [], []
    for i in range(STEPS):
        if i % ep.steps_per_epoch == 0:
            ep.begin_epoch()
        loss, logs = step()
        outs.append((loss.clone(), {k: torch.as_tensor(v).clone() for k, v in logs.items()}))
        flags.append(bool(wrapper.graphed) if wrapper else False)
    torch.cuda.synchronize()
    assert seg.global_step == STEPS
    params = [p.detach().clone() for p in seg.all_reduced_parameters()]
    return outs, params, wrapper, flags, seg


def _bits(t):
    return t.detach().reshape(-1).contiguous().cpu().view(torch.uint8)


def _hold(name, a, a2, g):
    """G equals A bit for bit where A' does; elsewhere it is no further from A than A' is."""
    assert a.shape == a2.shape == g.shape and a.dtype == g.dtype, name
    if torch.equal(_bits(a), _bits(a2)):
        assert torch.equal(_bits(a), _bits(g)), f"{name}: the eager pair repeats itself, the graphed run differs by {float((a.double() - g.double()).abs().max()):.3e}"
    else:
        pair, got = float((a.double() - a2.double()).abs().max()), float((a.double() - g.double()).abs().max())
        print(f"{name}: eager vs eager {pair:.3e}, graphed vs eager {got:.3e}")
        assert got <= pair, f"{name}: graphed vs eager {got:.3e} above the eager pair's own {pair:.3e}"


def _compare(kind, dev, over, monkeypatch):
    A = _run(kind, dev, False, over, monkeypatch)
    A2 = _run(kind, dev, False, over, monkeypatch)
    G = _run(kind, dev, True, over, monkeypatch)
    for i, ((la, ga), (la2, ga2), (lg, gg)) in enumerate(zip(A[0], A2[0], G[0])):
        print(f"{kind} {over} step {i}: loss eager {float(la)!r} graphed {float(lg)!r}")
        assert bool(torch.isfinite(la))
        _hold(f"loss of step {i}", la, la2, lg)
        assert set(ga) == set(ga2) == set(gg), (i, sorted(ga), sorted(gg))
        for k in ga:
            _hold(f"log {k} of step {i}", ga[k], ga2[k], gg[k])
    assert len(A[1]) == len(G[1]) >= 6
    for i, (pa, pa2, pg) in enumerate(zip(A[1], A2[1], G[1])):
        _hold(f"parameter {i} after step {STEPS}", pa, pa2, pg)
    # the host state the bookkeeping moves: the same in both routes
    from depthg_amd.graph_step import CAPTURE_KEY
    assert [getattr(A[4].cfg, k, None) for k in CAPTURE_KEY] == [getattr(G[4].cfg, k, None) for k in CAPTURE_KEY]
    return A, G


@pytest.mark.parametrize("kind", ["standin40", "dino"])
def test_graphed_steps_equal_the_eager_route(kind, dev, monkeypatch):
    """Four steps across an epoch boundary: the first is the eager warm-up the recording follows, the other three are replays."""
    A, G = _compare(kind, dev, {}, monkeypatch)
    assert G[2].captures == 1 and G[3] == [False, True, True, True]
    assert not any(k.startswith("hist/") for _, logs in G[0] for k in logs)
    # three steps moved the loss's scalars apart from step to step: the replays drew anew
    assert len({float(l) for l, _ in G[0]}) == STEPS


def test_a_decay_that_changes_the_key_records_again(dev, monkeypatch):
    """(a) fps_sample_decay changes feature_samples behind the step with global_step 2 (and, quirk Q9, behind step 0, in front of the
    first recording): two recordings, and the results match the eager route across the boundary."""
    over = dict(fps_sample_decay=True, fps_sample_decay_every_steps=2, fps_sample_decay_factor=0.8, fps_min_samples=2)
    A, G = _compare("standin40", dev, over, monkeypatch)
    assert G[4].cfg.feature_samples == A[4].cfg.feature_samples == 3          # 5 -> 4 behind step 0, 4 -> 3 behind step 2
    assert G[2].captures == 2 and G[3] == [False, True, True, False]


def test_a_histogram_step_runs_eagerly(dev, monkeypatch):
    """(b) hist_freq = 2: the step with global_step 2 runs eagerly on the same device state and its logs carry the three hist/ entries;
    the recording made behind step 0 serves the steps around it."""
    A, G = _compare("standin40", dev, dict(hist_freq=2), monkeypatch)
    assert G[2].captures == 1 and G[3] == [False, True, False, True]
    for i, (_, logs) in enumerate(G[0]):
        assert len([k for k in logs if k.startswith("hist/")]) == (3 if i == 2 else 0), (i, sorted(logs))


def test_a_failed_recording_is_reported_once_and_runs_eagerly(dev, monkeypatch, capsys):
    from depthg_amd import graph_step

    class Failing:
        def __init__(self, *a, **k):
            raise RuntimeError("recording refused by the test")
    A = _run("standin40", dev, False, {}, monkeypatch)
    A2 = _run("standin40", dev, False, {}, monkeypatch)
    monkeypatch.setattr(graph_step.torch.cuda, "graph", Failing)
    G = _run("standin40", dev, True, {}, monkeypatch, strict=False)
    err = capsys.readouterr().err
    assert err.count("recording the step failed") == 1 and "recording refused by the test" in err and "eagerly" in err
    assert G[2].captures == 0 and G[3] == [False] * STEPS
    for i, ((la, _), (la2, _), (lg, _)) in enumerate(zip(A[0], A2[0], G[0])):
        _hold(f"loss of step {i}", la, la2, lg)
    with pytest.raises(RuntimeError, match="recording refused by the test"):
        _run("standin40", dev, True, {}, monkeypatch, strict=True)


SIZES = [(120, 112), (112, 130), (128, 128), (150, 112), (112, 112), (140, 120), (113, 127), (131, 117)]


def test_train_command_with_graph_step(tmp_path):
    """(c) Three steps of `python -m depthg_amd.train --feature-cache float32 --sample-cache --graph-step` in a fresh process write
    last.pt and a log with three step lines."""
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    DF.make_directory(root, sizes=SIZES, split="train", n_classes=5)
    DF.make_directory(root, sizes=SIZES[:4], split="val", n_classes=5, seed=2)
    args = ["--data-dir", root, "--out", out, "--dataset", "directory", "--precompute-knns", "--feature-cache", "float32", "--sample-cache",
            "--graph-step", "res=112", "dim=70", "max_steps=3", "val_freq=2", "batch_size=2", "scalar_log_freq=1", "num_workers=2", "crop_type=~",
            "loader_crop_type=center", "num_neighbors=3", "use_depth=False", "depth_feat_correlation_loss=False", "depth_sampling=none",
            "dir_dataset_n_classes=5"]
    run = subprocess.run([sys.executable, "-m", "depthg_amd.train"] + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "3 step(s), 1 validation(s)" in run.stdout and "1 recording(s) of the step" in run.stdout
    assert "recording the step failed" not in run.stderr
    assert os.path.getsize(os.path.join(out, "last.pt")) > 0
    steps = [l for l in (json.loads(l) for l in open(os.path.join(out, "log.jsonl"))) if "val" not in l]
    assert [l["step"] for l in steps] == [1, 2, 3]
    for l in steps:
        assert l["loss/total"] == l["loss/total"] and abs(l["loss/total"]) < float("inf")
