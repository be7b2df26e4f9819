"""CPU-side checks of the reconstruction term (dg_recloss_*, ops.rec_loss_forward / rec_loss_backward, rec_loss.reconstruction_loss,
cfg.rec_weight in the segmenter): the exports, the C ABI's refusals, the CPU route and the float64 restatement's analytic gradients
against autograd, the refusals, and the segmenter's decoder and optimiser lists.  (The refusal of GPU tensors that are not float32
needs GPU tensors: tests/test_gpu_rec_loss.py.)"""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
import rec_loss_reference as R
from depthg_amd import rec_loss  # noqa: F401  (the module under test: without it nothing here can pass)
from depthg_amd.rec_loss import reconstruction_loss

NAMES = ["dg_recloss_workspace_bytes", "dg_recloss_forward", "dg_recloss_backward"]


def test_entry_points_are_declared_listed_and_exported():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [n for n in _lib.EXPORTS if "recloss" in n] == NAMES               # the header's order
    assert lib.dg_version() == _lib.DG_VERSION


def test_workspace_bytes():
    from depthg_amd import _lib
    lib = _lib.load()
    for B, D, C, (h, w) in list(R.SHAPES.values()) + [(32, 70, 384, (28, 28)), (1, 1, 1, (1, 1))]:
        need = lib.dg_recloss_workspace_bytes(B, D, C, h, w)
        # two norms and s per position, one double per tile of 64 positions, at least one partial of d W and d b
        assert need >= B * h * w * 12 + 8 * B * ((h * w + 63) // 64) + (C * D + C) * 4 and need % 256 == 0
    # far below one (B, C, h, w) tensor at the training shape
    assert lib.dg_recloss_workspace_bytes(32, 70, 384, 28, 28) < 32 * 384 * 28 * 28 * 4 // 4
    for bad in ((0, 5, 4, 4, 3), (2, 0, 4, 4, 3), (2, 5, 0, 4, 3), (2, 5, 4, -1, 3), (2, 5, 4, 4, 0), (2, 129, 4, 4, 4),
                (64, 70, 1024, 256, 256), (1, 70, 1 << 25, 1, 1)):
        assert lib.dg_recloss_workspace_bytes(*bad) == 0, bad


def _forward(B=2, D=8, C=12, h=4, w=4, ptr=16, scale=1.0, ws_bytes=1 << 30, **at):
    """dg_recloss_forward with dummy addresses: every case here is refused before anything is launched or dereferenced."""
    from depthg_amd import _lib
    lib = _lib.load()
    p = lambda k: ctypes.c_void_p(at.get(k, ptr))
    rc = lib.dg_recloss_forward(p("code"), p("feats"), p("weight"), p("bias"), p("keep"), scale, B, D, C, h, w, p("ws"), ws_bytes, p("loss"), None)
    return rc, lib.dg_last_error().decode()


def _backward(B=2, D=8, C=12, h=4, w=4, ptr=16, scale=1.0, ws_bytes=1 << 30, **at):
    from depthg_amd import _lib
    lib = _lib.load()
    p = lambda k: ctypes.c_void_p(at.get(k, ptr))
    rc = lib.dg_recloss_backward(p("code"), p("feats"), p("weight"), p("bias"), p("keep"), scale, p("ws"), ws_bytes, B, D, C, h, w, p("grad"),
                                 p("d_code"), p("d_weight"), p("d_bias"), None)
    return rc, lib.dg_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_any_launch():
    for call in (_forward, _backward):
        for kw in (dict(B=0), dict(D=0), dict(C=-3), dict(h=0), dict(w=-1)):
            rc, msg = call(**kw)
            assert rc == -1 and "positive" in msg, (call.__name__, kw, rc, msg)
        rc, msg = call(D=129)
        assert rc == -2 and "128" in msg
        for kw in (dict(B=64, C=1024, h=256, w=256), dict(B=1 << 20, h=1 << 10, w=1 << 10), dict(C=1 << 25, D=70)):
            rc, msg = call(**kw)
            assert rc == -2 and "2^31" in msg, (call.__name__, kw, rc, msg)
        rc, msg = call(ptr=0)
        assert rc == -1 and "null" in msg
        for kw in (dict(keep=0), ):                                           # the keep flags alone may be NULL ...
            rc, msg = call(ws_bytes=255, **kw)
            assert rc == -3 and "workspace" in msg
        for bad_scale in (0.0, -1.0, float("inf"), float("nan")):             # ... and with them the scale must be a scale
            rc, msg = call(scale=bad_scale)
            assert rc == -1 and "scale" in msg, (bad_scale, msg)
        for kw in (dict(ws=24), dict(code=18), dict(feats=6), dict(weight=10), dict(bias=17), dict(keep=22)):
            rc, msg = call(**kw)
            assert rc == -1 and "aligned" in msg, (call.__name__, kw, msg)
        rc, msg = call(ws_bytes=255)
        assert rc == -3 and "workspace" in msg
    assert _forward(loss=6)[0] == -1
    for kw in (dict(grad=18), dict(d_code=6), dict(d_weight=10), dict(d_bias=5)):
        assert _backward(**kw)[0] == -1


@pytest.mark.parametrize("shape,kind", R.CASES)
def test_analytic_gradients_match_float64_autograd(shape, kind):
    code, feats, weight, bias = (t.double() for t in R.operands(shape, kind))
    code.requires_grad_(True); weight.requires_grad_(True); bias.requires_grad_(True)
    loss = R.torch_chain(code, feats, weight, bias)
    loss.backward()
    t = R.truth(shape, kind)
    assert abs(float(loss.detach()) - t["loss"]) <= 1e-12
    if kind == "aligned":                    # the true gradient vanishes: nothing to be relative to
        assert abs(t["loss"] + 1.0) <= 1e-6 and float(t["d_code"].abs().max()) <= 1e-6
        return
    C, D = feats.shape[1], code.shape[1]
    for got, want in ((t["d_code"], code.grad), (t["d_weight"], weight.grad.reshape(C, D)), (t["d_bias"], bias.grad)):
        assert float((got - want).norm() / want.norm()) <= 1e-10


def test_restatement_follows_normalize_below_eps():
    """y = 0 exactly (code and bias zero) and f = 0 at two positions: s = 0 there, and autograd's gradient - the partner's unit vector
    over eps - is what the formulas give."""
    code, feats, weight, bias = (t.double().clone() for t in R.operands("ragged", "random"))
    bias.zero_()
    code[0, :, 1, 2] = 0
    feats[1, :, 3, 4] = 0
    t = R.chain(code, feats, weight, bias)
    assert float(t["s"][0, 1, 2]) == 0.0 and float(t["s"][1, 3, 4]) == 0.0 and float(t["norm_y"][0, 1, 2]) == 0.0
    code.requires_grad_(True); weight.requires_grad_(True); bias.requires_grad_(True)
    R.torch_chain(code, feats, weight, bias).backward()
    assert float(code.grad[0, :, 1, 2].abs().max()) > 1e7
    for got, want in ((t["d_code"], code.grad), (t["d_weight"], weight.grad.reshape(100, 70)), (t["d_bias"], bias.grad)):
        assert float((got - want).norm() / want.norm()) <= 1e-10


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.float64, 1e-10)])
@pytest.mark.parametrize("shape,kind", [("tiny", "random"), ("ragged", "random"), ("ragged", "dropped"), ("head", "scaled")])
def test_cpu_route_matches_the_restatement(shape, kind, dtype, tol):
    code, feats, weight, bias = (t.detach().clone().to(dtype) for t in R.operands(shape, kind))
    code.requires_grad_(True); weight.requires_grad_(True); bias.requires_grad_(True)
    loss = reconstruction_loss(code, feats, weight, bias)
    assert loss.dim() == 0 and loss.dtype == dtype
    loss.backward()
    t = R.truth(shape, kind)
    assert abs(float(loss.detach()) - t["loss"]) <= tol * t["mean_abs_s"]
    C, D = feats.shape[1], code.shape[1]
    for got, want in ((code.grad, t["d_code"]), (weight.grad.reshape(C, D), t["d_weight"]), (bias.grad, t["d_bias"])):
        assert float((got.double() - want).norm() / want.norm()) <= tol
    # a (C, D) weight view and a DeferredDropout are the same term
    from depthg_amd import ops
    i = R.inputs(shape, kind)
    with torch.no_grad():
        assert torch.equal(reconstruction_loss(code, feats, weight.reshape(C, D), bias), loss)
        if i["keep"] is not None:
            deferred = ops.DeferredDropout(i["raw"].to(dtype), i["keep"], i["scale"])
            assert torch.equal(reconstruction_loss(code, deferred, weight, bias), loss)


def test_refusals():
    code, feats, weight, bias = R.operands("tiny", "random")                  # (2,3,2,2), (2,5,2,2), (5,3,1,1), (5,)
    with pytest.raises(RuntimeError, match="feats"):
        reconstruction_loss(code, feats.clone().requires_grad_(True), weight, bias)
    with torch.no_grad():                                                     # (nothing to refuse when no graph is built)
        reconstruction_loss(code, feats.clone().requires_grad_(True), weight, bias)
    for bad in ((code[0], feats, weight, bias), (code, feats[:, :, 0], weight, bias)):
        with pytest.raises(ValueError, match=r"\(B, D, h, w\)"):
            reconstruction_loss(*bad)
    for bad in ((code[:1], feats, weight, bias), (code[:, :, :1], feats, weight, bias)):
        with pytest.raises(ValueError, match="batch size and the grid"):
            reconstruction_loss(*bad)
    for bad in ((code, feats, weight[:4], bias), (code, feats, weight[:, :2], bias), (code, feats, weight, bias[:4]),
                (code, feats, weight.reshape(3, 5), bias), (code, feats, weight[:, :, 0], bias)):
        with pytest.raises(ValueError, match="decoder"):
            reconstruction_loss(*bad)


def _segmenter(weight, **over):
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(4)
    return UnsupervisedSegmenter(5, default_segmenter_cfg(res=32, rec_weight=weight, **over))


def test_segmenter_builds_the_decoder_only_under_the_weight():
    m0, m1 = _segmenter(0.0), _segmenter(0.5)
    assert not hasattr(m0, "decoder") and not any("decoder" in k for k in m0.state_dict())
    assert isinstance(m1.decoder, torch.nn.Conv2d) and tuple(m1.decoder.weight.shape) == (384, 70, 1, 1) and tuple(m1.decoder.bias.shape) == (384,)
    s0, s1 = m0.state_dict(), m1.state_dict()
    assert set(s1) - set(s0) == {"decoder.weight", "decoder.bias"} and set(s0) <= set(s1)
    # built last: every other initial value is the weight-0 model's
    assert all(torch.equal(s0[k], s1[k]) for k in s0)
    assert [id(p) for p in m1.head_parameters()] == [id(p) for p in m1.net.parameters() if p.requires_grad]
    assert not any(p is q for p in m1.head_parameters() for q in m1.decoder.parameters())


@pytest.mark.parametrize("fused", [False, True])
def test_optimisers_and_the_all_reduce_list_hold_the_decoder_once(fused):
    m0, m1 = _segmenter(0.0, dg_fused_adam=fused), _segmenter(0.5, dg_fused_adam=fused)
    count = lambda params, t: sum(1 for p in params if p is t)
    for m, want in ((m0, 0), (m1, 1)):
        optims = m.configure_optimizers()
        stepped = [[p for g in o.param_groups for p in g["params"]] for o in optims]
        decoder = list(m.decoder.parameters()) if want else []
        assert len(stepped[0]) == len(m.head_parameters()) + 2 * want and len(stepped[1]) == 2 and len(stepped[2]) == 1
        for t in decoder:
            assert count(stepped[0], t) == 1 and count(stepped[1] + stepped[2], t) == 0
            assert count(m.all_reduced_parameters(), t) == 1
        assert [id(p) for p in m.all_reduced_parameters()] == [id(p) for ps in stepped for p in ps]      # the optimisers' order
        assert len(m.all_reduced_parameters()) == 9 + 2 * want


def test_training_step_names_the_fix_for_a_missing_decoder():
    m = _segmenter(0.0, correspondence_weight=0.0)
    m.cfg.rec_weight = 0.5                                                    # mutated after construction: no decoder was built
    assert m._decoder_parameters() == []

    def net(img):                                                             # (the check sits behind the featurizer pass)
        return torch.zeros(2, 384, 4, 4), torch.zeros(2, 70, 4, 4), None

    m.net.forward = net
    batch = {"img": torch.zeros(2, 3, 32, 32), "img_pos": torch.zeros(2, 3, 32, 32), "label": torch.zeros(2, 32, 32, dtype=torch.long),
             "depth": torch.ones(2, 1, 32, 32), "depth_pos": torch.ones(2, 1, 32, 32)}
    with pytest.raises(RuntimeError, match="before constructing UnsupervisedSegmenter"):
        m.training_step(batch, 0)
