"""CPU-side checks of the reconstruction term's gradient with respect to feats (dg_rec_feats_backward, dg_head_backward_input's
grad_feats_out, rec_loss.reconstruction_loss(feats_grad=True), cfg.dg_rec_feats_grad): the exports, the C ABI's refusals (which return before
any launch), the float64 restatement against autograd, the CPU route, and the segmenter's construction rule.  (The depth featurizer's
head has no CPU route, so a training_step with the key runs on the GPU only: tests/test_gpu_rec_feats.py.)"""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
import rec_feats_reference as F
import rec_loss_reference as R

NEW = {"dg_rec_feats_backward": 19, "dg_head_backward_input": 22}     # (the head's entry: keep3 and the two grad_feats_out among its 22)


def test_exports_are_declared_bound_and_built():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = _lib.load()
    for name, count in NEW.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^()]*)\)\s*;", code)
        assert proto, name
        assert len(proto.group(1).split(",")) == count, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == count and len(getattr(lib, name).argtypes) == count, name
    order = list(_lib.SIGNATURES)
    assert order.index("dg_rec_feats_backward") == order.index("dg_recloss_backward") + 1
    for suffix in ("_pair", "_add", "_add_pair"):                              # one input-gradient entry: its variants are folded into it
        gone = "dg_head_backward_input" + suffix
        assert gone not in _lib.EXPORTS and gone not in header and not hasattr(lib, gone), gone
    assert lib.dg_version() == _lib.DG_VERSION == 119


def _backward(B=2, D=8, C=12, h=4, w=4, ptr=16, scale=1.0, ws_bytes=1 << 30, **at):
    """dg_rec_feats_backward with dummy addresses: every case here is refused before anything is launched or dereferenced."""
    from depthg_amd import _lib
    lib = _lib.load()
    p = lambda k: ctypes.c_void_p(at.get(k, ptr))
    rc = lib.dg_rec_feats_backward(p("code"), p("feats"), p("weight"), p("bias"), p("keep"), scale, p("ws"), ws_bytes, B, D, C, h, w, p("grad"),
                                   p("d_code"), p("d_weight"), p("d_bias"), p("d_feats"), None)
    return rc, lib.dg_last_error().decode()


def test_rec_feats_backward_refuses_bad_arguments_before_any_launch():
    for kw in (dict(B=0), dict(D=0), dict(C=-3), dict(h=0), dict(w=-1)):
        rc, msg = _backward(**kw)
        assert rc == -1 and "positive" in msg, (kw, rc, msg)
    rc, msg = _backward(D=129)
    assert rc == -2 and "128" in msg
    rc, msg = _backward(B=64, C=1024, h=256, w=256)
    assert rc == -2 and "2^31" in msg
    for kw in (dict(ptr=0), dict(d_feats=0), dict(code=0), dict(grad=0), dict(ws=0)):
        rc, msg = _backward(**kw)
        assert rc == -1 and "null" in msg, (kw, msg)
    # the three parameter-side gradients are given together or not at all
    for kw in (dict(d_code=0), dict(d_weight=0), dict(d_bias=0), dict(d_code=0, d_weight=0), dict(d_weight=0, d_bias=0)):
        rc, msg = _backward(**kw)
        assert rc == -1 and "together" in msg, (kw, msg)
    for kw in (dict(d_code=0, d_weight=0, d_bias=0), dict(keep=0), dict()):    # ... and these are legal: refused for the workspace alone
        rc, msg = _backward(ws_bytes=255, **kw)
        assert rc == -3 and "workspace" in msg, (kw, msg)
    for bad_scale in (0.0, -1.0, float("inf"), float("nan")):
        rc, msg = _backward(scale=bad_scale)
        assert rc == -1 and "scale" in msg, (bad_scale, msg)
    for kw in (dict(ws=24), dict(code=18), dict(feats=6), dict(keep=22), dict(grad=18), dict(d_code=6), dict(d_weight=10), dict(d_bias=5),
               dict(d_feats=18)):
        rc, msg = _backward(**kw)
        assert rc == -1 and "aligned" in msg, (kw, msg)


def test_head_backward_input_add_refuses_bad_arguments_before_any_launch():
    from depthg_amd import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    x, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)                       # never dereferenced
    B, C, D, P = 2, 64, 16, 9
    ws, iws = lib.dg_head_workspace_bytes(B, C, D, P), lib.dg_head_input_workspace_bytes(C, D)
    ws2 = lib.dg_head_workspace_bytes(2 * B, C, D, P)

    def single(C=C, D=D, P=P, w1=x, k3=x, g=x, gf=x, wsb=ws, dx=x, iw=x, iwb=iws):
        return lib.dg_head_backward_input(B, C, D, P, w1, x, x, x, k3, 1.0, x, g, null, gf, null, x, wsb, dx, null, iw, iwb, null)

    def pair(g2=x, gf=x, gf2=x, dx=x, dx2=x, wsb=ws2, B=B):
        return lib.dg_head_backward_input(B, C, D, P, x, x, x, x, x, 1.0, x, x, g2, gf, gf2, x, wsb, dx, dx2, x, iws, null)

    assert single(C=776) == UNSUPPORTED and single(D=129) == UNSUPPORTED and single(P=0) == INVALID
    for kw in (dict(w1=null), dict(g=null), dict(dx=null), dict(iw=null)):
        assert single(**kw) == INVALID, kw
    assert single(gf=ctypes.c_void_p(4100)) == INVALID and b"aligned" in lib.dg_last_error()
    assert single(k3=ctypes.c_void_p(4098)) == INVALID
    assert single(wsb=ws - 1) == WORKSPACE and single(iwb=iws - 1) == WORKSPACE
    assert single(gf=null, wsb=ws - 1) == WORKSPACE and single(k3=null, wsb=ws - 1) == WORKSPACE       # both may be NULL
    assert pair(g2=null) == INVALID and pair(dx=null, dx2=null, gf=null, gf2=null) == INVALID and pair(B=0) == INVALID
    assert pair(dx=null) == INVALID and b"grad_feats_out of a pass" in lib.dg_last_error()             # an addend without its pass
    assert pair(dx=null, gf=null, wsb=ws2 - 1) == WORKSPACE and pair(gf=null, gf2=null, wsb=ws2 - 1) == WORKSPACE


@pytest.mark.parametrize("shape,kind", F.CASES)
def test_analytic_d_feats_matches_float64_autograd(shape, kind):
    err = F.check_formula(shape, kind)
    if kind == "aligned":                    # the true gradient vanishes: nothing to be relative to
        assert err <= 1e-12 and float(F.truth(shape, kind).abs().max()) <= 1e-6
        return
    assert err <= 1e-10, err
    t, i = F.truth(shape, kind), F.inputs(shape, kind)
    assert t.shape == i["raw"].shape and bool(torch.isfinite(t).all())
    if kind == "dropped":
        dropped = i["keep"] == 0
        assert bool(dropped.any()) and bool((t[dropped] == 0).all())
    if kind == "small_f":                    # b' = 0 and nf = eps: the partner's unit vector over eps, times -1/N
        B, _, _, (h, w) = R.SHAPES[shape]
        y = torch.nn.functional.conv2d(i["code"].double(), i["weight"].double(), i["bias"].double())
        for b, yy, xx in ((0, 0, 0), (B - 1, h - 1, w - 1)):
            assert float(i["feats"][b, :, yy, xx].abs().max()) == 0.0
            want = -y[b, :, yy, xx] / y[b, :, yy, xx].norm() / R.EPS / (B * h * w)
            assert float((t[b, :, yy, xx] - want).norm() / want.norm()) <= 1e-12 and float(want.abs().max()) > 1e6


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.float64, 1e-10)])
@pytest.mark.parametrize("shape,kind", [("tiny", "random"), ("ragged", "random"), ("ragged", "dropped"), ("head", "scaled"), ("ragged", "small_f")])
def test_cpu_route_hands_feats_its_gradient(shape, kind, dtype, tol):
    from depthg_amd import ops
    from depthg_amd.rec_loss import reconstruction_loss
    i = F.inputs(shape, kind)
    code, weight, bias = (i[k].detach().clone().to(dtype).requires_grad_(True) for k in ("code", "weight", "bias"))
    feats = i["feats"].detach().clone().to(dtype).requires_grad_(True)
    with pytest.raises(RuntimeError, match="no gradient for `feats`"):        # without the keyword: refused, text unchanged
        reconstruction_loss(code, feats, weight, bias)
    loss = reconstruction_loss(code, feats, weight, bias, feats_grad=True)
    loss.backward()
    want = F.d_feats(i["code"], i["feats"], i["weight"], i["bias"])
    assert float((feats.grad.double() - want).norm() / want.norm()) <= tol
    t = R.chain(i["code"], i["feats"], i["weight"], i["bias"])
    assert float((code.grad.double() - t["d_code"]).norm() / t["d_code"].norm()) <= tol
    # the keyword alone changes nothing for a feats that does not ask
    plain = reconstruction_loss(code.detach(), feats.detach(), weight.detach(), bias.detach())
    assert torch.equal(reconstruction_loss(code.detach(), feats.detach(), weight.detach(), bias.detach(), feats_grad=True), plain)
    if i["keep"] is not None:                # the maps of a DeferredDropout get the un-dropped map's gradient
        raw = i["raw"].detach().clone().to(dtype).requires_grad_(True)
        deferred = ops.DeferredDropout(raw, i["keep"], i["scale"])
        with pytest.raises(RuntimeError, match="no gradient for `feats`"):
            reconstruction_loss(code, deferred, weight, bias)
        reconstruction_loss(code, deferred, weight, bias, feats_grad=True).backward()
        assert float((raw.grad.double() - F.truth(shape, kind)).norm() / F.truth(shape, kind).norm()) <= tol
        assert bool((raw.grad[i["keep"] == 0] == 0).all())


def test_head_keyword_needs_input_grad():
    from depthg_amd.head import ProjectionHead
    head = ProjectionHead(64, 16).train()
    with pytest.raises(ValueError, match="input_grad=True"):
        head(torch.zeros(2, 64, 3, 3), feats_grad=True)
    with pytest.raises(ValueError, match="input_grad=True"):
        head.forward_pair(torch.zeros(2, 64, 3, 3), torch.zeros(2, 64, 3, 3), feats_grad=True)


def test_segmenter_constructs_with_the_key_and_refuses_without():
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    assert default_segmenter_cfg().dg_rec_feats_grad is False
    for guidance in ("sum", "cross_attn"):
        with pytest.raises(ValueError, match="rec_weight.*dg_rec_feats_grad"):
            UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance=guidance, rec_weight=0.5))
        seg = UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance=guidance, rec_weight=0.5, dg_rec_feats_grad=True))
        assert isinstance(seg.decoder, torch.nn.Conv2d) and seg.net.cfg.dg_rec_feats_grad is True
        seg.cfg.dg_rec_feats_grad = False    # changed after construction: refused in front of the step's first launch
        with pytest.raises(ValueError, match="dg_rec_feats_grad"):
            seg.training_step({"img": None, "img_pos": None, "label": None, "depth": None, "depth_pos": None})
    # under the other guidances and the plain arch the key changes nothing that is built
    for over in (dict(arch="dino_depth", guidance="none"), dict(arch="dino_depth", guidance="concat"), dict()):
        torch.manual_seed(2)
        a = UnsupervisedSegmenter(5, default_segmenter_cfg(rec_weight=0.5, **over))
        torch.manual_seed(2)
        b = UnsupervisedSegmenter(5, default_segmenter_cfg(rec_weight=0.5, dg_rec_feats_grad=True, **over))
        assert list(a.state_dict()) == list(b.state_dict())
        assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
