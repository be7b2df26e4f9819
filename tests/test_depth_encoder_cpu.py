"""The fused depth encoder without a GPU: exports and prototypes, refusals through the C ABI, the workspace bound, the CPU route, the
float64 references and the construction-time flag."""
import ctypes
import os
import re
import warnings

import pytest
import torch

from tests import depth_encoder_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dg_depthenc_workspace_bytes", "dg_depthenc_forward", "dg_depthenc_backward")


def _lib():
    from depthg_amd import _lib
    return _lib, _lib.load()


def test_exports_and_prototypes():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name)
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^()]*)\)\s*;", code)
        assert m, f"{name}: no prototype in include/depthg_corr.h"
        params = [p for p in m.group(2).split(",")]
        restype, argtypes = L.SIGNATURES[name]
        assert len(params) == len(argtypes), name
        assert restype is (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int)
    doc = header[header.index("The three-stage depth encoder"):header.index("size_t dg_depthenc_workspace_bytes")]
    for cite in ("src/modules.py:497-506", ":557", ":562-563", ":619-631"):
        assert cite in doc, cite
    assert lib.dg_version() == L.DG_VERSION == 119


A16 = 4096        # a non-null, 16-byte aligned address that is never dereferenced: every refusal comes before any launch


def _fwd(lib, *, depth=A16, params=(A16,) * 10, residual=0, rhw=None, B=2, C=384, h=4, w=4, dhw=None, out=A16, ws=A16, ws_bytes=1 << 40):
    rhw = rhw or (h, w)
    dhw = dhw or (8 * h, 8 * w)
    return lib.dg_depthenc_forward(depth, *params, residual, rhw[0], rhw[1], B, C, h, w, dhw[0], dhw[1], out, ws, ws_bytes, None)


def _bwd(lib, *, depth=A16, params=(A16,) * 10, gout=A16, B=2, C=384, h=4, w=4, dhw=None, grads=(A16,) * 10, ws=A16, ws_bytes=1 << 40):
    dhw = dhw or (8 * h, 8 * w)
    return lib.dg_depthenc_backward(depth, *params, gout, B, C, h, w, dhw[0], dhw[1], *grads, ws, ws_bytes, None)


def test_refusals_through_the_c_abi():
    L, lib = _lib()
    err = lambda: lib.dg_last_error().decode()
    for call in (_fwd, _bwd):
        assert call(lib, C=100) == -2 and "multiple of 64" in err()
        assert call(lib, C=832) == -2 and "768" in err()
        assert call(lib, dhw=(32, 24)) == -1 and "32x32" in err()
        assert call(lib, B=0) == -1
        assert call(lib, depth=0) == -1 and "null" in err()
        assert call(lib, depth=A16 + 2) == -1 and "aligned" in err()
        assert call(lib, ws=A16 + 8) == -1 and "aligned" in err()
        assert call(lib, ws_bytes=1024) == -3 and "dg_depthenc_workspace_bytes" in err()
    assert _fwd(lib, residual=A16, rhw=(4, 5)) == -1 and "residual" in err()
    assert _bwd(lib, grads=(A16,) * 9 + (0,)) == -1 and "gradient" in err()
    assert lib.dg_depthenc_workspace_bytes(2, 100, 4, 4, 1) == 0 and lib.dg_depthenc_workspace_bytes(0, 384, 4, 4, 1) == 0


def test_python_refusals():
    from depthg_amd import depth_encoder
    from depthg_amd.featurizer import make_depth_downscaling
    stack = R.make_stack(384, 0)
    with pytest.raises(ValueError, match="five-stage"):
        depth_encoder(torch.rand(1, 1, 32, 32), make_depth_downscaling(768))
    with pytest.raises(RuntimeError, match="no gradient for the depth map"):
        depth_encoder(torch.rand(1, 1, 8, 8, requires_grad=True), stack)
    with pytest.raises(ValueError, match="multiples of 8"):
        depth_encoder(torch.rand(1, 1, 12, 8), stack)
    with pytest.raises(ValueError, match=r"residual must be \(B, C, h, w\) = \(1, 384, 1, 2\)"):
        depth_encoder(torch.rand(1, 1, 8, 16), stack, torch.zeros(1, 384, 2, 1))


def test_workspace_bound():
    """Activation sections (bf16 x2 and d a2, whole tiles of 32 positions) <= twice the result's bytes (whole tiles too); the rest is
    the four weight images and the partial sums, each at its documented size."""
    L, lib = _lib()
    up = lambda n: (n + 255) // 256 * 256
    for B, C, h, w in ((32, 384, 28, 28), (1, 384, 1, 1)):
        N = B * h * w
        tiles = (N + 31) // 32
        out_bytes = tiles * 32 * C * 4
        packs = 2 * (up(128 * 256 * 2) + up(C * 512 * 2))
        blocks, s2, s3 = min((tiles + 1) // 2, 512), min((tiles + 3) // 4, 64), min((tiles + 3) // 4, 32)
        partials = up(blocks * 832 * 4) + up(s2 * 128 * 256 * 4) + up(s3 * (C * 512 + 2 * C) * 4)
        bwd, fwd = lib.dg_depthenc_workspace_bytes(B, C, h, w, 1), lib.dg_depthenc_workspace_bytes(B, C, h, w, 0)
        assert fwd == packs // 2
        assert 0 < bwd <= 2 * out_bytes + packs + partials
        assert bwd - packs - partials == 2 * up(tiles * 512 * 32 * 2)      # nothing of stage-1 size: exactly the two bf16 sections
        if N % 32 == 0:
            assert bwd <= 2 * N * C * 4 + packs + partials


@pytest.mark.parametrize("with_residual", [False, True])
def test_cpu_route_is_the_stack_bit_for_bit(with_residual):
    from depthg_amd import depth_encoder
    stack = R.make_stack(384, 3)
    depth = torch.rand(2, 1, 16, 24, generator=torch.Generator().manual_seed(1))
    res = torch.randn(2, 384, 2, 3, generator=torch.Generator().manual_seed(2)) if with_residual else None
    want = stack(depth) if res is None else res + stack(depth)
    got = depth_encoder(depth, stack, res)
    assert torch.equal(got, want)
    assert torch.equal(depth_encoder(depth[:, 0], stack, res), want)
    got.square().sum().backward()
    g1 = [p.grad.clone() for p in stack.parameters()]
    stack.zero_grad()
    want.square().sum().backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(g1, stack.parameters()))


def _case(B, h, w, C, seed):
    g = torch.Generator().manual_seed(seed)
    stack = R.make_stack(C, seed)
    return stack, torch.rand(B, 1, 8 * h, 8 * w, generator=g), torch.randn(B, C, h, w, generator=g), torch.randn(B, C, h, w, generator=g)


def test_float64_restatement_equals_autograd():
    for B, h, w, C in ((2, 3, 5, 128), (1, 1, 1, 64)):
        stack, depth, gout, res = _case(B, h, w, C, 7)
        out_t, grads_t = R.truth(stack, depth, gout, res)
        out_c, grads_c = R.chain(R.stack_params(stack), depth, gout, res)          # rnd = identity: the yardstick restates the truth
        assert float((out_c - out_t).abs().max()) <= 1e-12 * float(out_t.abs().max())
        for name, a, b in zip(R.NAMES, grads_c, grads_t):
            assert a.shape == b.shape, name
            assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1.0), name


def test_yardstick_rounds_and_stays_close():
    stack, depth, gout, res = _case(2, 3, 5, 128, 8)
    out_t, grads_t = R.truth(stack, depth, gout)
    out_y, grads_y = R.yardstick(R.stack_params(stack), depth, gout)
    assert torch.equal(out_y, out_y.float().double())
    for name, y, t in (("out", out_y, out_t), *zip(R.NAMES, grads_y, grads_t)):
        rel = float((y - t).norm() / t.norm())
        assert 0 < rel < 3e-2, (name, rel)
    R.check("self", out_y, out_t, out_y)


def _build(cls, cfg, *args):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cls(cfg.dim, cfg, *args)


def test_flag_default_and_state_dict():
    from depthg_amd.featurizer import DinoFeaturizerWithDepth
    from depthg_amd.segmenter import StandInFeaturizerWithDepth, default_segmenter_cfg
    assert default_segmenter_cfg().dg_fused_depth_encoder is False
    tiny = dict(dg_dino_vit_kwargs=dict(embed_dim=384, depth=1), dim=16, arch="dino_depth", guidance="sum")
    for cls in (DinoFeaturizerWithDepth, StandInFeaturizerWithDepth):
        off, on = _build(cls, default_segmenter_cfg(**tiny)), _build(cls, default_segmenter_cfg(dg_fused_depth_encoder=True, **tiny))
        absent = default_segmenter_cfg(**tiny)
        del absent.dg_fused_depth_encoder                    # a cfg that predates the key: the torch route
        gone = _build(cls, absent)
        assert on.fused_depth_encoder and not off.fused_depth_encoder and not gone.fused_depth_encoder
        so, sn, sg = off.state_dict(), on.state_dict(), gone.state_dict()
        assert list(so) == list(sn) == list(sg)
        assert all(torch.equal(so[k], sn[k]) and torch.equal(so[k], sg[k]) for k in so)
        assert [(n, p.requires_grad) for n, p in off.named_parameters()] == [(n, p.requires_grad) for n, p in on.named_parameters()]


def test_flag_with_the_five_stage_stack_is_refused():
    from depthg_amd.featurizer import DinoFeaturizerWithDepth
    from depthg_amd.segmenter import default_segmenter_cfg
    cfg = default_segmenter_cfg(dg_dino_vit_kwargs=dict(embed_dim=192, depth=1, num_heads=3), dim=16, arch="dino_depth", guidance="sum",
                                dg_fused_depth_encoder=True)
    with pytest.raises(ValueError, match="n_feats"):
        _build(DinoFeaturizerWithDepth, cfg)
    cfg.dg_fused_depth_encoder = False
    _build(DinoFeaturizerWithDepth, cfg)
