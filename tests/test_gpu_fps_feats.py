"""The feature-aware farthest point sampling (cfg.dg_fps_feats; ops.fps_feats_coords, k_fps_feats) on the GPU against the numpy
restatement of tests/fps_feats_reference.py, on the margin inputs of its CASES (every round's two largest running distances are at
least 1e-3 apart, so neither float32 order of the channel sum can flip a choice: indices are compared exactly, coordinates bit for
bit).  The kernel-level tests run twice, the second time with every buffer handed to the library pre-filled with 0xFF bytes
(ops.POISON, as under DG_POISON=1)."""
import numpy as np
import pytest
import torch

import fps_feats_reference as R

pytestmark = pytest.mark.gpu

PARITY = ["5x5", "7x9", "8x8_all", "16x16", "28x28"]          # (h, w, C, S) = (5,5,3,2) (7,9,17,3) (8,8,1,8) (16,16,64,5) (28,28,384,11; B = 2)
_WANT = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(params=[False, True], ids=["plain", "poisoned"])
def poison(request):
    from depthg_amd import ops
    old = ops.POISON
    ops.POISON = request.param
    yield request.param
    ops.POISON = old


def want(name):
    """(depth, feats, S, coords, inds) of a case: the restatement runs once per case and its results are shared."""
    if name not in _WANT:
        seeds, C, h, w, H, W, S = R.CASES[name]
        depth, feats = R.margin_inputs(seeds, C, h, w, H, W, S, flat_depth=name.startswith("flat_depth"))
        coords, inds = R.sample(depth, feats, S, np.float32)
        for a in (depth, feats, coords, inds):
            a.setflags(write=False)
        _WANT[name] = (depth, feats, S, coords, inds)
    return _WANT[name]


def _bits(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_restatement(name, dev, poison):
    from depthg_amd import ops
    depth, feats, S, coords, inds = want(name)
    d, f = torch.from_numpy(depth.copy()).to(dev), torch.from_numpy(feats.copy()).to(dev)
    got_c, got_i = ops.fps_feats_coords(d, f, f.shape[-2:], S, return_inds=True)
    assert got_i.dtype == torch.int32 and got_i.shape == inds.shape and got_c.shape == coords.shape
    assert np.array_equal(got_i.cpu().numpy().astype(np.int64), inds), "selection order"
    assert np.array_equal(got_c.cpu().numpy().view(np.uint32), coords.view(np.uint32)), "coordinates, bit for bit"
    assert torch.equal(_bits(ops.fps_feats_coords(d, f, f.shape[-2:], S)), _bits(got_c))          # without the index output


def test_pair_launch_equals_two_single_launches_and_repeats_itself(dev, poison):
    from depthg_amd import ops
    depth, feats, S, _, _ = want("28x28")
    d, f = torch.from_numpy(depth.copy()).to(dev), torch.from_numpy(feats.copy()).to(dev)
    dp, fp = d.flip(0).contiguous(), (f.flip(0) * 1.5).contiguous()
    both = ops.fps_feats_coords_pair(d, dp, f, fp, (28, 28), S)
    assert both.shape == (4, S, S, 2)
    assert torch.equal(_bits(both[:2]), _bits(ops.fps_feats_coords(d, f, (28, 28), S)))
    assert torch.equal(_bits(both[2:]), _bits(ops.fps_feats_coords(dp, fp, (28, 28), S)))
    assert torch.equal(_bits(both), _bits(ops.fps_feats_coords_pair(d, dp, f, fp, (28, 28), S)))       # two calls give equal bits
    # more than 1024 points: two and four points per thread (kernel against kernel: no margin is asked of these inputs)
    g = torch.Generator().manual_seed(1)
    for h, w in ((33, 32), (50, 47)):
        d2, f2 = torch.rand(1, 1, 2 * h, 2 * w, generator=g).to(dev) + 0.1, torch.randn(1, 5, h, w, generator=g).to(dev)
        c, i = ops.fps_feats_coords(d2, f2, (h, w), 7, return_inds=True)
        c2, i2 = ops.fps_feats_coords(d2, f2, (h, w), 7, return_inds=True)
        assert torch.equal(_bits(c), _bits(c2)) and torch.equal(i, i2)
        srt = np.sort(i[0].cpu().numpy().astype(np.int64))
        assert len(set(srt.tolist())) == 49 and srt[0] == 0 and srt[-1] < h * w
        rows = (srt // w).astype(np.float32) / np.float32(h) * np.float32(2) - np.float32(1)          # (on the host: IEEE division)
        cols = (srt % w).astype(np.float32) / np.float32(w) * np.float32(2) - np.float32(1)
        assert np.array_equal(c[0].reshape(-1, 2).cpu().numpy(), np.stack([rows, cols], -1))


def test_degenerate_inputs_give_distinct_valid_indices(dev, poison):
    """The 0 / 0 rule: an all-zero depth map, a constant feature map, and both - the restatement's selections."""
    from depthg_amd import ops
    rs = np.random.RandomState(0)
    for depth, feats in ((np.zeros((2, 1, 12, 12), np.float32), rs.standard_normal((2, 5, 6, 6)).astype(np.float32)),
                         (rs.uniform(0.5, 2, (2, 1, 12, 12)).astype(np.float32), np.full((2, 5, 6, 6), 0.25, np.float32)),
                         (np.zeros((2, 1, 6, 6), np.float32), np.zeros((2, 2, 6, 6), np.float32))):
        for S in (3, 6):
            c, i = ops.fps_feats_coords(torch.from_numpy(depth).to(dev), torch.from_numpy(feats).to(dev), (6, 6), S, return_inds=True)
            i = i.cpu().numpy()
            for row in i:
                assert len(set(row.tolist())) == S * S and row.min() >= 0 and row.max() < 36 and row[0] == 0
            assert bool(torch.isfinite(c).all()) and float(c.min()) >= -1 and float(c.max()) < 1
    assert i[0].tolist() == list(range(36))            # nothing tells the points apart: index order


def test_the_feature_term_decides(dev, poison):
    """Flat depth (the points form a plane): the selection leaves the depth-only sampler's and equals the restatement's."""
    from depthg_amd import ops
    depth, feats, S, coords, inds = want("flat_depth")
    d, f = torch.from_numpy(depth.copy()).to(dev), torch.from_numpy(feats.copy()).to(dev)
    c, i = ops.fps_feats_coords(d, f, (6, 6), S, return_inds=True)
    assert np.array_equal(i.cpu().numpy().astype(np.int64), inds) and np.array_equal(c.cpu().numpy().view(np.uint32), coords.view(np.uint32))
    assert not torch.equal(c, ops.fps_coords(d, (6, 6), S))


def test_python_routes_refuse_by_name(dev):
    from depthg_amd import ops
    d, f = torch.ones(2, 1, 12, 12, device=dev), torch.ones(2, 8, 6, 6, device=dev)
    with pytest.raises(ValueError, match="`feats`"):
        ops.fps_feats_coords(d, f.half(), (6, 6), 3)
    with pytest.raises(ValueError, match="`depth`"):
        ops.fps_feats_coords(d.double(), f, (6, 6), 3)
    with pytest.raises(ValueError, match="`feats`"):
        ops.fps_feats_coords(d, f.transpose(2, 3), (6, 6), 3)
    with pytest.raises(ValueError, match="`feats_pos`"):
        ops.fps_feats_coords_pair(d, d, f, f.transpose(2, 3), (6, 6), 3)
    with pytest.raises(ValueError, match="features"):
        ops.fps_feats_coords(d, f, (5, 5), 2)
    with pytest.raises(ValueError, match="must match"):
        ops.fps_feats_coords_pair(d, d[:1], f, f, (6, 6), 3)
    with pytest.raises(RuntimeError, match="cannot sample"):
        ops.fps_feats_coords(d, f, (6, 6), 7)


def _batch(dev, seed=0, hw=40, n_classes=5, B=2):
    g = torch.Generator().manual_seed(seed)
    return {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
            "label": torch.randint(-1, n_classes, (B, hw, hw), generator=g).to(dev),
            "depth": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev),
            "depth_pos": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev)}


def _step(dev, **over):
    """One seeded training_step at 40 x 40 (a 5 x 5 grid, S = 4) -> (loss, logs, what _draw_coords was handed and returned)."""
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(4)
    m = UnsupervisedSegmenter(5, default_segmenter_cfg(res=40, feature_samples=4, fps_sample_decay=False, hist_freq=None, **over)).to(dev)
    m.train()
    seen = []
    loss_fn = m.contrastive_corr_loss_fn
    inner = loss_fn._draw_coords

    def spy(orig_feats, orig_feats_pos, sal, sal_pos, depth, depth_pos, *a, **k):
        out = inner(orig_feats, orig_feats_pos, sal, sal_pos, depth, depth_pos, *a, **k)
        seen.append((orig_feats.detach().clone(), orig_feats_pos.detach().clone(), depth.detach().clone(), depth_pos.detach().clone(),
                     out[0].detach().clone(), out[1].detach().clone()))
        return out

    loss_fn._draw_coords = spy
    torch.manual_seed(9)
    loss, logs = m.training_step(_batch(dev), 0)
    torch.cuda.synchronize()
    return loss, logs, seen


def test_training_step_with_the_key_on_and_off(dev):
    from depthg_amd import ops
    loss, logs, seen = _step(dev, depth_sampling="fps_depth_feat", dg_fps_feats=True)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in logs.values())
    assert len(seen) == 1
    f, fp, d, dp, c1, c2 = seen[0]
    assert f.shape == (2, 384, 5, 5) and c1.shape == c2.shape == (2, 4, 4, 2)
    both = ops.fps_feats_coords_pair(d, dp, f.float().contiguous(), fp.float().contiguous(), (5, 5), 4)
    assert torch.equal(c1, both[:2]) and torch.equal(c2, both[2:])
    # off (and absent): the parent's route, the depth-only sampler
    for over in (dict(dg_fps_feats=False), {}):
        loss0, logs0, seen0 = _step(dev, depth_sampling="fps_depth_feat", **over)
        f, fp, d, dp, c1, c2 = seen0[0]
        both = ops.fps_coords_pair(d, dp, (5, 5), 4)
        assert bool(torch.isfinite(loss0)) and torch.equal(c1, both[:2]) and torch.equal(c2, both[2:])
    # ... which is what 'fps' draws, with the key set or not
    loss1, _, seen1 = _step(dev, depth_sampling="fps", dg_fps_feats=True)
    assert torch.equal(seen1[0][4], c1) and torch.equal(seen1[0][5], c2) and bool(torch.isfinite(loss1))


def test_recorded_steps_equal_the_eager_route(dev, monkeypatch):
    """Three GraphedTrainStep replays behind the eager warm-up, with the key on, at the sizes of tests/test_gpu_graph_step.py (whose
    runs and bit-for-bit comparison these are)."""
    import test_gpu_graph_step as GS
    from depthg_amd import ops
    calls = []
    inner = ops.fps_feats_coords_pair
    monkeypatch.setattr(ops, "fps_feats_coords_pair", lambda *a: (calls.append(1), inner(*a))[1])
    A, G = GS._compare("standin40", dev, dict(depth_sampling="fps_depth_feat", dg_fps_feats=True), monkeypatch)
    assert G[2].captures == 1 and G[3] == [False, True, True, True]
    assert len(calls) >= 4 + 4 + 1                    # two eager runs of four steps; the graphed run's eager step (replays call nothing)
    assert len({float(l) for l, _ in G[0]}) == GS.STEPS
