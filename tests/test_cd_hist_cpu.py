"""The cd histograms (dg_corr_cd_hist / ops.corr_cd_hist / ContrastiveCorrelationLoss.cd_histograms) without a GPU: the export and
its binding, the refusals of the host layer, the reference bin rule against torch.histc, and the cfg keys the segmenter reads."""
import inspect

import numpy as np
import pytest
import torch

import cd_hist_reference as R


def test_library_exports_cd_hist_and_binding_declares_it():
    from depthg_amd import _lib
    assert "dg_corr_cd_hist" in _lib.SIGNATURES
    # at the header's position: behind the materialise entry points
    assert _lib.EXPORTS.index("dg_corr_cd_hist") == _lib.EXPORTS.index("dg_corr_materialize_shared") + 1
    lib = _lib.load()
    assert hasattr(lib, "dg_corr_cd_hist")
    assert lib.dg_version() == _lib.DG_VERSION          # the number is unchanged: one more export under it
    assert len(_lib.SIGNATURES["dg_corr_cd_hist"][1]) == 11


def test_corr_cd_hist_refuses_cpu_tensors():
    from depthg_amd import ops
    desc = ops.make_desc(2, 64, 70, 14, 14, 11, 5, pointwise=True, zero_clamp=True, stabalize=False, depth_term=False, need_grad=False,
                         shared_coords=False, shifts=(0.1, 0.2, 0.3, 0.4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.corr_cd_hist(desc, torch.zeros(1024, dtype=torch.uint8), 0, 2)


def test_cd_histograms_before_any_forward_raises():
    from depthg_amd import ContrastiveCorrelationLoss
    from oracle import depthg_oracle as O
    with pytest.raises(RuntimeError, match="none has run"):
        ContrastiveCorrelationLoss(O.default_cfg(feature_samples=4)).cd_histograms()


def test_library_refuses_bad_arguments_without_a_gpu():
    """The argument checks come before anything touches the device: they run here with dummy pointers."""
    import ctypes
    from depthg_amd import _lib, ops
    lib = _lib.load()
    mk = lambda shared: ops.make_desc(2, 64, 70, 14, 14, 14, 3, pointwise=True, zero_clamp=True, stabalize=False, depth_term=False,
                                      need_grad=False, shared_coords=shared, identity_grid=shared, shifts=(0.1, 0.2, 0.3, 0.4))
    desc = mk(False)
    big = ctypes.c_size_t(1 << 40)
    p = ctypes.c_void_p(256)          # never dereferenced: every call below is refused first
    call = lambda d, first, count, perms, nbins, lo, hi: lib.dg_corr_cd_hist(ctypes.byref(d), first, count, perms, nbins, lo, hi, p, p, big, None)
    for args, text in (((desc, -1, 1, None, 64, -1.0, 1.0), b"first=-1"),
                       ((desc, 0, 6, None, 64, -1.0, 1.0), b"outside [0,5)"),
                       ((desc, 5, 1, None, 64, -1.0, 1.0), b"outside [0,5)"),
                       ((desc, 0, 0, None, 64, -1.0, 1.0), b"outside [0,5)"),
                       ((desc, 0, 2, None, 0, -1.0, 1.0), b"nbins=0"),
                       ((desc, 0, 2, None, 257, -1.0, 1.0), b"nbins=257"),
                       ((desc, 0, 2, None, 64, 1.0, 1.0), b"lo < hi"),
                       ((desc, 0, 2, None, 64, 0.5, -0.5), b"lo < hi"),
                       ((desc, 0, 2, None, 64, -1.0, float("inf")), b"lo < hi"),
                       ((desc, 0, 2, None, 64, float("nan"), 1.0), b"lo < hi"),
                       ((mk(True), 0, 3, None, 64, -1.0, 1.0), b"batch maps")):
        assert call(*args) < 0, args[1:]
        assert text in lib.dg_last_error(), (args[1:], lib.dg_last_error())


def test_reference_bin_rule_is_histc_inside_the_range():
    g = torch.Generator().manual_seed(7)
    bins, lo, hi = 64, -1.0, 1.0
    v = (torch.rand(200_000, generator=g) * 2 - 1).double()
    edges = torch.from_numpy(R.interior_edges(bins, lo, hi))          # multiples of 1/32: exact
    v = torch.cat([v, edges, torch.tensor([lo, hi, hi, lo], dtype=torch.float64)])
    want = torch.histc(v, bins=bins, min=lo, max=hi).numpy().astype(np.int64)
    got = R.clamped_histc(v.numpy(), bins, lo, hi)
    assert got.sum() == v.numel() and np.array_equal(got, want)
    assert got[-1] >= 2 and got[0] >= 2                              # hi itself is in the last bin
    # an exact edge belongs to the bin on its right
    assert np.array_equal(R.clamped_histc(edges.numpy(), bins, lo, hi), np.r_[0, np.ones(bins - 1, dtype=np.int64)])
    # an odd bin count on a range that is not centred
    v7 = v[(v >= -0.5) & (v <= 0.9)]
    assert np.array_equal(R.clamped_histc(v7.numpy(), 7, -0.5, 0.9), torch.histc(v7, bins=7, min=-0.5, max=0.9).numpy().astype(np.int64))


def test_reference_bin_rule_clamps_what_histc_drops():
    bins, lo, hi = 8, -1.0, 1.0
    inside = np.linspace(-0.99, 0.99, 37)
    outside = np.array([-1.0000001, -3.0, 1.0000001, 2.5, 1e30])
    v = np.concatenate([inside, outside])
    got = R.clamped_histc(v, bins, lo, hi)
    dropped = torch.histc(torch.from_numpy(v), bins=bins, min=lo, max=hi).numpy().astype(np.int64)
    assert dropped.sum() == inside.size and got.sum() == v.size
    diff = got - dropped
    assert diff[0] == 2 and diff[-1] == 3 and not diff[1:-1].any()
    # the helpers of the bound
    assert np.array_equal(R.below_edges(got), np.cumsum(got)[:-1])
    m = R.edge_mass(np.array([-0.5, -0.5 + 1e-4, -0.5 - 2e-3, 0.0]), 8, lo, hi, 1e-3)
    assert m[1] == 2 and m[3] == 1 and m.sum() == 3


def test_segmenter_cfg_keys():
    from depthg_amd import segmenter
    cfg = segmenter.default_segmenter_cfg()
    assert cfg.hist_freq == 100                                       # the reference's shipped default
    assert not hasattr(cfg, "dg_hist_bins")                           # optional, build-side: read with getattr
    # (the step reads the key through its plan, training.step_plan, and takes the histograms in its correspondence stage)
    from depthg_amd import training
    assert 'getattr(cfg, "dg_hist_bins", 64)' in inspect.getsource(training.step_plan)
    assert "step_plan(" in inspect.getsource(segmenter.UnsupervisedSegmenter.training_step)
    src = inspect.getsource(segmenter.UnsupervisedSegmenter._correspondence_term)
    assert "cd_histograms(bins=plan.hist_bins)" in src
