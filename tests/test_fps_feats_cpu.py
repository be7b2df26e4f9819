"""The feature-aware farthest point sampling (cfg.dg_fps_feats) without a GPU: the numpy restatement against the indices the reference's
own fps_depth_feats returned (tests/golden/fps_feats_*.npz, scripts/make_fps_feats_fixtures.py), the margin every committed input
holds, the export and its binding, the C entry's refusals, the loss's route and the recorded step's key."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fps_feats_reference as R
from conftest import ROOT, load_golden


def case_inputs(name):
    """(fixture, depth, feats, S) of a committed case: the stored inputs, or the ones re-drawn from the recorded seeds - held to the
    fixture's seeds, shape and checksum either way."""
    fx = load_golden(f"fps_feats_{name}.npz")
    seeds, C, h, w, H, W, S = R.CASES[name]
    assert tuple(int(s) for s in fx["seeds"]) == tuple(seeds) and [int(v) for v in fx["shape"]] == [len(seeds), C, h, w, H, W, S]
    depth, feats = R.margin_inputs(seeds, C, h, w, H, W, S, flat_depth=name.startswith("flat_depth"))
    if "depth" in fx:
        assert np.array_equal(fx["depth"], depth) and np.array_equal(fx["feats"], feats), "the stored inputs are not the seeds' draw"
    chk = np.asarray([depth.astype(np.float64).sum(), np.abs(depth.astype(np.float64)).sum(), feats.astype(np.float64).sum(),
                      np.abs(feats.astype(np.float64)).sum()])
    assert np.allclose(chk, fx["input_checksum"], rtol=1e-12, atol=1e-9), "the seeded inputs differ from the ones the reference ran on"
    return fx, depth, feats, S


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_reproduces_the_reference_and_the_margin_holds(name):
    fx, depth, feats, S = case_inputs(name)
    c32, i32 = R.sample(depth, feats, S, np.float32)
    c64, i64, margin = R.sample(depth, feats, S, np.float64, want_margin=True)
    assert np.array_equal(i32, fx["sample_inds"]), "float32 restatement against the reference's sample_inds"
    assert np.array_equal(i64, fx["sample_inds"]), "float64 restatement against the reference's sample_inds"
    assert margin >= R.MARGIN and margin == pytest.approx(float(fx["margin"]), rel=1e-9)
    assert np.array_equal(c32, c64) and c32.shape == (len(i32), S, S, 2) and c32.dtype == np.float32
    for row in i32:
        assert len(set(row.tolist())) == S * S and row[0] == 0


def test_restatement_on_degenerate_inputs_selects_distinct_points():
    """The 0 / 0 rule: a zero depth map (all points coincide in space) and a constant feature map (... in feature space)."""
    rs = np.random.RandomState(0)
    for depth, feats in ((np.zeros((1, 1, 12, 12), np.float32), rs.standard_normal((1, 5, 6, 6)).astype(np.float32)),
                         (rs.uniform(0.5, 2, (1, 1, 12, 12)).astype(np.float32), np.full((1, 5, 6, 6), 0.25, np.float32)),
                         (np.zeros((1, 1, 6, 6), np.float32), np.zeros((1, 2, 6, 6), np.float32))):
        _, inds = R.sample(depth, feats, 6)
        assert sorted(inds[0].tolist()) == list(range(36))
        _, inds = R.sample(depth, feats, 3)
        assert len(set(inds[0].tolist())) == 9
    # nothing to tell the points apart: index order
    assert inds[0].tolist() == list(range(9))


def test_export_binding_and_version():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in ("dg_fps_feats_coords", "dg_fps_feats_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    restype, argtypes = _lib.SIGNATURES["dg_fps_feats_coords"]
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert restype is ctypes.c_int and argtypes == [vp] * 4 + [i32] * 7 + [vp, vp, vp, ctypes.c_size_t, vp]
    assert lib.dg_fps_feats_workspace_bytes(4, 28, 28) >= 4 * 28 * 28 * 4
    m = re.search(r"#define\s+DG_VERSION\s+(\d+)\b", header)
    assert lib.dg_version() == _lib.DG_VERSION == int(m.group(1))
    assert "1124-1180" in header and "dg_fps_feats" in header          # the header cites the reference's lines and names the key


def _call(depth=16, depth_pos=0, feats=16, feats_pos=0, B=2, C=8, H=12, W=12, h=6, w=6, S=3, coords=16, inds=0, ws=16, ws_bytes=1 << 20):
    from depthg_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p
    rc = lib.dg_fps_feats_coords(p(depth), p(depth_pos), p(feats), p(feats_pos), B, C, H, W, h, w, S, p(coords), p(inds), p(ws), ws_bytes, None)
    return rc, lib.dg_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_any_launch():
    for kw in (dict(depth=0), dict(feats=0), dict(coords=0), dict(ws=0)):
        rc, msg = _call(**kw)
        assert rc == -1 and "null" in msg, (kw, rc, msg)
    for kw in (dict(depth=18), dict(feats=17), dict(coords=6), dict(inds=2), dict(ws=3), dict(depth_pos=18, feats_pos=16)):
        rc, msg = _call(**kw)
        assert rc == -1 and "aligned" in msg, (kw, rc, msg)
    for kw in (dict(depth_pos=16), dict(feats_pos=16)):
        rc, msg = _call(**kw)
        assert rc == -1 and "together" in msg, (kw, rc, msg)
    for kw in (dict(C=0), dict(C=-3)):
        rc, msg = _call(**kw)
        assert rc == -1 and "C=" in msg, (kw, rc, msg)
    rc, msg = _call(S=7)                                     # 49 points from a 6 x 6 map
    assert rc == -1 and "cannot sample" in msg
    for kw in (dict(B=0), dict(h=0), dict(S=0), dict(H=5), dict(W=5)):
        rc, msg = _call(**kw)
        assert rc == -1 and "dimensions" in msg, (kw, rc, msg)
    rc, msg = _call(h=65, w=64, H=130, W=128)                # the grid limit of dg_fps_coords
    assert rc == -2 and "4096" in msg
    rc, msg = _call(C=16385)
    assert rc == -2 and "C=" in msg
    rc, msg = _call(ws_bytes=2 * 36 * 4 - 1)
    assert rc == -3 and "workspace" in msg
    rc, msg = _call(depth_pos=16, feats_pos=16, ws_bytes=4 * 36 * 4 - 1)       # the pair needs the pooled maps of 2B images
    assert rc == -3 and "workspace" in msg


def test_python_routes_refuse_by_name():
    from depthg_amd import ops
    d, f = torch.ones(2, 1, 12, 12), torch.ones(2, 8, 6, 6)
    with pytest.raises(RuntimeError, match="`depth` must live on the GPU"):
        ops.fps_feats_coords(d, f, (6, 6), 3)
    with pytest.raises(RuntimeError, match="`depth` must live on the GPU"):
        ops.fps_feats_coords_pair(d, d, f, f, (6, 6), 3)
    # (the refusals of a GPU tensor of another type or layout: tests/test_gpu_fps_feats.py)


def _loss(monkeypatch, **over):
    from depthg_amd import ContrastiveCorrelationLoss, ops
    cfg = SimpleNamespace(feature_samples=3, use_salience=False, depth_sampling="fps_depth_feat", **over)
    calls = []

    def record(name):
        def fn(*a):
            calls.append((name, a))
            n = a[0].shape[0] * (2 if name.endswith("pair") else 1)
            return torch.zeros(n, 3, 3, 2)
        return fn
    for name in ("fps_coords", "fps_coords_pair", "fps_feats_coords", "fps_feats_coords_pair"):
        monkeypatch.setattr(ops, name, record(name))
    return ContrastiveCorrelationLoss(cfg), calls


def test_loss_route(monkeypatch):
    f, fp = torch.randn(2, 8, 6, 6), torch.randn(2, 8, 6, 6)
    d, dp = torch.rand(2, 1, 12, 12), torch.rand(2, 1, 12, 12)
    # the key absent or False: 'fps_depth_feat' stays 'fps' (quirk Q13)
    for over in ({}, dict(dg_fps_feats=False)):
        loss, calls = _loss(monkeypatch, **over)
        c1, c2, shared = loss._draw_coords(f, fp, None, None, d, dp)
        assert [n for n, _ in calls] == ["fps_coords_pair"] and calls[0][1][0] is d and calls[0][1][1] is dp and not shared
    # on: the new op, with orig_feats / orig_feats_pos as handed in
    loss, calls = _loss(monkeypatch, dg_fps_feats=True)
    c1, c2, shared = loss._draw_coords(f, fp, None, None, d, dp)
    (name, args), = calls
    assert name == "fps_feats_coords_pair" and not shared and c1.shape == c2.shape == (2, 3, 3, 2)
    assert args[0] is d and args[1] is dp and args[2] is f and args[3] is fp and tuple(args[4]) == (6, 6) and args[5] == 3
    # maps of two sizes: two single calls
    loss, calls = _loss(monkeypatch, dg_fps_feats=True)
    fp7 = torch.randn(2, 8, 7, 7)
    loss._draw_coords(f, fp7, None, None, d, dp)
    assert [n for n, _ in calls] == ["fps_feats_coords", "fps_feats_coords"] and calls[0][1][1] is f and calls[1][1][1] is fp7
    # 'fps' never reads the key
    loss, calls = _loss(monkeypatch, dg_fps_feats=True)
    loss.cfg.depth_sampling = "fps"
    loss._draw_coords(f, fp, None, None, d, dp)
    assert [n for n, _ in calls] == ["fps_coords_pair"]
    # depth missing: the mode's own refusal, before any op
    loss, calls = _loss(monkeypatch, dg_fps_feats=True)
    with pytest.raises(AttributeError):
        loss._draw_coords(f, fp, None, None, None, None)
    assert calls == []


def test_capture_key_and_default_cfg():
    from depthg_amd.graph_step import CAPTURE_KEY
    from depthg_amd.segmenter import default_segmenter_cfg
    assert "dg_fps_feats" in CAPTURE_KEY and len(set(CAPTURE_KEY)) == len(CAPTURE_KEY)
    assert default_segmenter_cfg().dg_fps_feats is False
