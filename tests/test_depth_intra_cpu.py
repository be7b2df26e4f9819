"""DepthContrastiveCorrelationLoss (cfg.use_depth_only_intra) without a GPU: the float64 restatement against the reference's recorded
outputs and against the oracle's plain loss, the new export in header, library and binding, every refusal with its reason, and the
segmenter's default."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import depth_intra_reference as R
from oracle import depthg_oracle as O

import depthg_amd
from depthg_amd import _lib, ops
from depthg_amd.loss import ContrastiveCorrelationLoss, DepthContrastiveCorrelationLoss
from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg

FX = load_golden("depth_intra.npz")
CASES = [str(c) for c in FX["cases"]]


def fixture_cfg(name, **over):
    p = name + "_"
    pw, zc, st = (bool(v) for v in FX[p + "cfg_flags"])
    s, w, (S, N) = FX[p + "cfg_shifts"], FX[p + "cfg_weights"], FX[p + "dims"]
    return O.default_cfg(**{**dict(feature_samples=int(S), neg_samples=int(N), pointwise=pw, zero_clamp=zc, stabalize=st,
                                   depth_feat_correlation_loss=False, pos_intra_shift=float(s[0]), pos_inter_shift=float(s[1]),
                                   neg_inter_shift=float(s[2]), pos_intra_weight=float(w[0]), pos_inter_weight=float(w[1]),
                                   neg_inter_weight=float(w[2]), correspondence_weight=float(w[3])), **over})


def fixture_inputs(name):
    T = lambda k: torch.from_numpy(FX[name + "_" + k])
    return T("feats"), T("feats_pos"), T("code"), T("code_pos"), T("aug"), T("coords1"), T("coords2"), list(T("perms"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_class(name):
    """float32 rounding of the reference's own run: 2e-6 absolute on means of O(0.1), 1e-5 on un-reduced elements and gradients."""
    cfg = fixture_cfg(name)
    out, total, g, gp = R.forward_backward_f64(cfg, *fixture_inputs(name))
    p = name + "_"
    for i, key in ((0, "pos_intra_loss"), (2, "pos_inter_loss")):
        assert abs(float(out[i]) - float(FX[p + key])) < 2e-6, key
    assert abs(float(total) - float(FX[p + "total"])) < 2e-6
    for i, key in ((1, "pos_intra_cd"), (3, "pos_inter_cd"), (4, "neg_inter_loss"), (5, "neg_inter_cd")):
        assert np.abs(out[i].numpy() - FX[p + key]).max() < 1e-5, key
    for got, key in ((g, "grad_code"), (gp, "grad_code_pos")):
        want = FX[p + key].astype(np.float64)
        assert np.linalg.norm(got.numpy() - want) / np.linalg.norm(want) < 1e-5, key


@pytest.mark.parametrize("name", CASES)
def test_restatement_with_the_same_map_is_the_oracles_plain_loss(name):
    cfg = fixture_cfg(name)
    f, fp, c, cp, _, c1, c2, perms = fixture_inputs(name)
    out = R.forward(cfg, f, fp, c, cp, f, c1, c2, perms)
    want = O.forward(cfg, f.double(), fp.double(), c.double(), cp.double(), coords1=c1.double(), coords2=c2.double(), perms=perms)
    # (the oracle forms the sample position in float32, as grid_sample does on float32 coordinates; the restatement hands float64
    #  coordinates to grid_sample.  A float32 position on a map of <= 7 pixels is off by <= 2^-22 of a pixel; neighbouring pixels of
    #  the randn maps differ by a few units, so a sampled vector of norm ~ sqrt(C) moves by ~1e-6 of itself and a cosine by a few
    #  1e-6: 1e-5, a decade below the least the second map moves the intra loss by, asserted next)
    for a, b in zip(out, want):
        assert float((a - b).abs().max()) < 1e-5
    # and the second map matters: the intra loss moves, nothing else does
    out2 = R.forward(cfg, f, fp, c, cp, fixture_inputs(name)[4], c1, c2, perms)
    assert abs(float(out2[0] - out[0])) > 1e-4
    for i in (1, 2, 3, 4, 5):
        assert torch.equal(out2[i], out[i])


def test_export_is_in_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    for name in ("dg_corr_forward_intra_feats", "dg_corr_workspace_bytes_intra_feats"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
    assert "src/modules.py:1370-1463" in header and ":1427-1438" in header
    assert "intra_feats" in inspect.signature(ops.corr_forward).parameters and depthg_amd.DepthContrastiveCorrelationLoss is DepthContrastiveCorrelationLoss
    assert issubclass(DepthContrastiveCorrelationLoss, ContrastiveCorrelationLoss)


def _desc(**over):
    kw = dict(pointwise=True, zero_clamp=True, stabalize=False, depth_term=False, need_grad=True, shared_coords=False,
              shifts=(0.1, 0.1, 0.4, 0.0))
    dims = dict(B=2, C=64, D=16, h=8, w=8, S=5, n_neg=2)
    for k in list(over):
        if k in dims:
            dims[k] = over.pop(k)
    kw.update(over)
    return ops.make_desc(dims["B"], dims["C"], dims["D"], dims["h"], dims["w"], dims["S"], dims["n_neg"], **kw)


def _forward_rc(desc, intra=1):
    """The entry's return code on fake non-null pointers: every refusal comes before the first launch."""
    one = ctypes.c_void_p(256)
    rc = _lib.load().dg_corr_forward_intra_feats(ctypes.byref(desc), one, one, one, one, None, one, one, one, 0, 0, None,
                                                 one if intra else None, one, one, 1 << 40, None)
    return rc, _lib.load().dg_last_error().decode()


@pytest.mark.parametrize("over, word", [
    (dict(identity_grid=True, shared_coords=True, S=8), "DG_IDENTITY_GRID"),
    (dict(shared_coords=True), "DG_SHARED_COORDS"),
    (dict(line_grid=True), "DG_LINE_GRID"),
    (dict(depth_term=True, depth_hw=(16, 16)), "DG_DEPTH_TERM"),
    (dict(code_hw=(15, 15)), "code maps"),
])
def test_c_abi_refusals_name_their_reason(over, word):
    desc = _desc(**over)
    rc, msg = _forward_rc(desc)
    assert rc == -2 and word in msg and "dg_corr_forward_intra_feats" in msg, (rc, msg)     # DG_ERR_UNSUPPORTED
    assert _lib.load().dg_corr_workspace_bytes_intra_feats(ctypes.byref(desc)) == 0


def test_c_abi_refuses_a_null_map_and_sizes_the_extra_operand():
    desc = _desc()
    rc, msg = _forward_rc(desc, intra=0)
    assert rc == -2 and "intra_feats is null" in msg, (rc, msg)
    lib = _lib.load()
    for d in (desc, _desc(S=14, h=14, w=14), _desc(S=12, h=14, w=14, C=72, D=70, n_neg=5, need_grad=False)):
        plain, intra = lib.dg_corr_workspace_bytes(ctypes.byref(d)), lib.dg_corr_workspace_bytes_intra_feats(ctypes.byref(d))
        assert 0 < plain < intra             # the existing query's result is what it was (tests/test_loss_workspace_cpu.py pins it)


def _maps(B=2, C=64, D=16, hw=8, **kw):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(B, C, hw, hw), r(B, C, hw, hw), None, None, r(B, D, hw, hw), r(B, D, hw, hw), r(B, C, hw, hw), r(B, C, hw, hw)


def test_python_refusals_name_the_fix():
    cfg = O.default_cfg(feature_samples=5, neg_samples=2, depth_feat_correlation_loss=False)
    loss = DepthContrastiveCorrelationLoss(cfg)
    assert loss.takes_deferred_dropout((8, 8)) is False
    with pytest.raises(ValueError, match="at most 768 channels"):
        loss(*_maps(C=776))
    m = list(_maps())
    m[0] = ops.DeferredDropout(m[0], torch.ones(2, 64), 1.0)
    with pytest.raises(ValueError, match=r"materialize\(\)"):
        loss(*m)
    m = list(_maps())
    m[6] = m[6][:, :32]
    with pytest.raises(RuntimeError, match="depth_aug_feats.*shape of orig_feats"):
        loss(*m)
    m = list(_maps())
    m[7] = m[7].long()
    with pytest.raises(ValueError, match="depth_aug_feats_pos.*floating-point"):
        loss(*m)
    for key, word in (("depth_feat_correlation_loss", "depth_feat_correlation_loss = False"), ("dg_graph_safe", "dg_graph_safe = False")):
        bad = DepthContrastiveCorrelationLoss(O.default_cfg(feature_samples=5, neg_samples=2, **{"depth_feat_correlation_loss": False, key: True}))
        with pytest.raises(ValueError, match=word):
            bad(*_maps())
    with pytest.raises(RuntimeError, match="must live on the GPU|no CPU path"):      # everything valid: the library is the next stop
        loss(*_maps())


def test_segmenter_default_and_refusals():
    cfg = default_segmenter_cfg(dino_patch_size=8, dim=16)
    assert not hasattr(cfg, "use_depth_only_intra")
    seg = UnsupervisedSegmenter(5, cfg)
    assert type(seg.contrastive_corr_loss_fn) is ContrastiveCorrelationLoss and seg.depth_only_intra is False
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(dim=16, use_depth_only_intra=False))
    assert type(seg.contrastive_corr_loss_fn) is ContrastiveCorrelationLoss
    with pytest.raises(ValueError, match="no depth-augmented features"):
        UnsupervisedSegmenter(5, default_segmenter_cfg(dim=16, use_depth_only_intra=True, depth_feat_correlation_loss=False))
    with pytest.raises(ValueError, match="cfg.lhp"):
        UnsupervisedSegmenter(5, default_segmenter_cfg(dim=16, use_depth_only_intra=True, arch="dino_depth", guidance="sum", lhp=True,
                                                       depth_feat_correlation_loss=False))
    with pytest.raises(ValueError, match="depth_feat_correlation_loss"):
        UnsupervisedSegmenter(5, default_segmenter_cfg(dim=16, use_depth_only_intra=True, arch="dino_depth", guidance="sum"))
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(dim=16, use_depth_only_intra=True, arch="dino_depth", guidance="sum",
                                                         depth_feat_correlation_loss=False))
    assert type(seg.contrastive_corr_loss_fn) is DepthContrastiveCorrelationLoss
