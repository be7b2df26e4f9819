"""CPU-side checks of the depth-guided featurizer (cfg.arch "dino_depth") and of the head's d image_feat entries: the exports, their
refusals (which return before any launch), DinoFeaturizerWithDepth's modules / state dict / requires_grad pattern, LayerNorm2d, the
float64 restatement of d image_feat against torch autograd, and the segmenter's refusals and unchanged default."""
import ctypes
import os
import re
import warnings

import pytest
import torch
import torch.nn as nn

import head_input_grad_reference as R
import head_margin_inputs as H
from conftest import ROOT

NEW_EXPORTS = ("dg_head_input_workspace_bytes", "dg_head_backward_input")
# one entry per operation, the widest argument list each: the second pass's tensors and the feats_out addend are NULL where absent
HEAD_ENTRIES = {"dg_head_forward": 23, "dg_head_backward": 22, "dg_head_backward_input": 22}
FOLDED_VARIANTS = {"dg_head_forward": ("_pair",), "dg_head_backward": ("_pair",), "dg_head_backward_input": ("_pair", "_add", "_add_pair"),
                   "dg_fps_coords": ("_pair",), "dg_super_perms": ("_seeded", "_state")}
TINY_VIT = dict(embed_dim=384, depth=1)


def tiny_cfg(**over):
    from depthg_amd.segmenter import default_segmenter_cfg
    return default_segmenter_cfg(dg_dino_vit_kwargs=dict(TINY_VIT), dim=16, **over)


def build(cls, cfg, seed=0):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cls(cfg.dim, cfg)


def test_exports_are_declared_bound_and_built():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name, count in HEAD_ENTRIES.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^()]*)\)\s*;", code)
        assert proto and len(proto.group(1).split(",")) == count, name
        assert len(_lib.SIGNATURES[name][1]) == count and len(getattr(lib, name).argtypes) == count, name
    for name, suffixes in FOLDED_VARIANTS.items():
        for gone in (name + s for s in suffixes):
            assert gone not in _lib.EXPORTS and gone not in header and not hasattr(lib, gone), gone
    assert lib.dg_head_input_workspace_bytes(384, 70) >= 2 * 384 * (70 + 384)
    assert lib.dg_head_input_workspace_bytes(384, 70) % 1024 == 0          # whole fragment tiles
    assert lib.dg_head_input_workspace_bytes(769, 70) == 0 and lib.dg_head_input_workspace_bytes(380, 70) == 0
    assert lib.dg_head_input_workspace_bytes(384, 129) == 0


def test_c_abi_refusals_return_before_any_launch():
    from depthg_amd import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    x = ctypes.c_void_p(4096)                                             # never dereferenced: every call below returns in its checks
    null = ctypes.c_void_p(0)
    B, C, D, P = 2, 64, 16, 9
    ws, iws = lib.dg_head_workspace_bytes(B, C, D, P), lib.dg_head_input_workspace_bytes(C, D)
    ws2 = lib.dg_head_workspace_bytes(2 * B, C, D, P)

    def single(C=C, D=D, P=P, w1=x, w2a=x, hidden=x, g=x, wsp=x, wsb=ws, dx=x, iw=x, iwb=iws):
        return lib.dg_head_backward_input(B, C, D, P, w1, w2a, x, x, null, 1.0, hidden, g, null, null, null, wsp, wsb, dx, null, iw, iwb, null)

    def pair(g2=x, dx=x, dx2=x, wsb=ws2, B=B):
        return lib.dg_head_backward_input(B, C, D, P, x, x, x, x, null, 1.0, x, x, g2, null, null, x, wsb, dx, dx2, x, iws, null)

    assert single(C=776) == UNSUPPORTED and single(C=60) == UNSUPPORTED and single(D=129) == UNSUPPORTED
    assert single(P=0) == INVALID
    for kw in (dict(w1=null), dict(g=null), dict(dx=null), dict(iw=null)):
        assert single(**kw) == INVALID, kw
    assert single(hidden=null) == INVALID                                  # a nonlinear call without `hidden`
    assert single(wsp=null) == INVALID
    assert single(wsb=ws - 1) == WORKSPACE and single(iwb=iws - 1) == WORKSPACE
    assert b"workspace" in lib.dg_last_error()
    assert pair(g2=null) == INVALID and pair(dx=null, dx2=null) == INVALID
    assert pair(wsb=ws2 - 1) == WORKSPACE and pair(B=0) == INVALID


def test_layernorm2d_is_its_formula():
    from depthg_amd.featurizer import LayerNorm2d
    torch.manual_seed(1)
    ln = LayerNorm2d(7).double()
    assert ln.eps == 1e-6
    with torch.no_grad():
        ln.weight.copy_(torch.randn(7)); ln.bias.copy_(torch.randn(7))
    x = torch.randn(3, 7, 5, 4, dtype=torch.float64)
    u = x.mean(1, keepdim=True)
    var = ((x - u) ** 2).sum(1, keepdim=True) / 7                          # biased variance over the channels
    want = ln.weight.view(1, 7, 1, 1) * (x - u) / torch.sqrt(var + 1e-6) + ln.bias.view(1, 7, 1, 1)
    assert torch.allclose(ln(x), want, rtol=1e-13, atol=1e-13)


DEPTH_KEYS_384 = {
    "depth_downscaling.0.weight": (64, 1, 2, 2), "depth_downscaling.0.bias": (64,),
    "depth_downscaling.1.weight": (64,), "depth_downscaling.1.bias": (64,),
    "depth_downscaling.3.weight": (128, 64, 2, 2), "depth_downscaling.3.bias": (128,),
    "depth_downscaling.4.weight": (128,), "depth_downscaling.4.bias": (128,),
    "depth_downscaling.6.weight": (384, 128, 2, 2), "depth_downscaling.6.bias": (384,),
    "cross_attn.in_proj_weight": (1152, 384), "cross_attn.in_proj_bias": (1152,),
    "cross_attn.out_proj.weight": (384, 384), "cross_attn.out_proj.bias": (384,),
    "no_depth_embed.weight": (1, 384),
}
TRAINED = {"none": (), "concat": (), "sum": ("depth_downscaling",), "cross_attn": ("depth_downscaling", "cross_attn")}


@pytest.mark.parametrize("guidance", ["none", "concat", "sum", "cross_attn"])
def test_depth_featurizer_modules_and_state_dict(guidance):
    from depthg_amd.featurizer import DinoFeaturizer, DinoFeaturizerWithDepth
    plain = build(DinoFeaturizer, tiny_cfg())
    net = build(DinoFeaturizerWithDepth, tiny_cfg(arch="dino_depth", guidance=guidance))
    sd, base = net.state_dict(), plain.state_dict()
    assert set(sd) == set(base) | set(DEPTH_KEYS_384)
    assert {k: tuple(sd[k].shape) for k in DEPTH_KEYS_384} == DEPTH_KEYS_384
    for k in base:                                                         # the depth modules are built after the head: same draws
        assert torch.equal(sd[k], base[k]), k
    assert isinstance(net.depth_downscaling[2], nn.GELU) and isinstance(net.depth_downscaling[5], nn.GELU)
    assert net.depth_downscaling[1].eps == 1e-6 and net.depth_downscaling[0].stride == (2, 2)
    assert isinstance(net.cross_attn, nn.MultiheadAttention) and net.cross_attn.num_heads == 8
    assert net.cross_attn.dropout == 0.1 and not net.cross_attn.batch_first
    # a state dict written under those names loads strictly
    other = {k: torch.randn_like(v) for k, v in sd.items()}
    net.load_state_dict(other, strict=True)
    assert all(torch.equal(net.state_dict()[k], other[k]) for k in other)
    # requires_grad: the head, and the depth modules the guidance touches in training
    for name, p in net.named_parameters():
        top = name.split(".")[0]
        want = top in ("cluster1", "cluster2") or top in TRAINED[guidance]
        assert p.requires_grad == want, (guidance, name)
    assert set(net.depth_parameters()) == set(DEPTH_KEYS_384)


def test_depth_featurizer_refuses_unknown_guidance_and_defaults_to_none():
    from depthg_amd.featurizer import DinoFeaturizerWithDepth
    with pytest.raises(ValueError, match="guidance"):
        build(DinoFeaturizerWithDepth, tiny_cfg(arch="dino_depth", guidance="product"))
    cfg = tiny_cfg(arch="dino_depth")
    del cfg.guidance
    assert build(DinoFeaturizerWithDepth, cfg).guidance == "none"


def test_five_stage_stack_for_other_widths():
    from depthg_amd.featurizer import LayerNorm2d, make_depth_downscaling
    seq = make_depth_downscaling(768)
    assert [i for i, m in enumerate(seq) if isinstance(m, nn.Conv2d)] == [0, 3, 6, 9, 12]
    assert [i for i, m in enumerate(seq) if isinstance(m, LayerNorm2d)] == [1, 4, 7, 10]
    assert [seq[i].out_channels for i in (0, 3, 6, 9, 12)] == [64, 128, 256, 512, 768]
    assert seq(torch.zeros(1, 1, 64, 64)).shape == (1, 768, 2, 2)


@pytest.mark.parametrize("case", [R.SMALL_EVAL, R.SMALL_PAIR, H.case_by_id("odd-15x15"), H.case_by_id("linear-pair-grouped")],
                         ids=lambda c: c.id)
def test_manual_input_gradient_restates_autograd(case):
    """dx_manual with rnd = identity against torch autograd through a plain-torch head with the same keep masks, to 1e-12"""
    inp = R.case_inputs(case)
    if case.B > 8:                                                        # (the formula does not depend on the batch: a slice of it)
        inp = H.Inputs(inp.feat[:4], tuple(k[:4] for k in inp.keeps), *inp[2:8], inp.up[:4])
    nl = inp.w2a is not None
    f = inp.feat.double().requires_grad_(True)
    drop = lambda i: f if inp.keeps is None else f * (inp.keeps[i].double() * H.SCALE)[:, :, None, None]
    conv = lambda x, w, b: torch.nn.functional.conv2d(x, w.double()[:, :, None, None], b.double())
    code = conv(drop(0), inp.w1, inp.b1)
    if nl:
        code = code + conv(torch.relu(conv(drop(1), inp.w2a, inp.b2a)), inp.w2b, inp.b2b)
    (code * inp.up.double()).sum().backward()
    got = R.dx_manual(inp, lambda t: t)
    assert float((got - f.grad).abs().max()) <= 1e-12 * float(f.grad.abs().max())
    assert torch.allclose(R.dx_truth(inp), f.grad, rtol=0, atol=1e-12 * float(f.grad.abs().max()))
    # the yardstick (bf16 operands) is a real, small error
    pre = R.pre_activation(inp)
    y = H.tensor_errors(R.dx_manual(inp, H.to_bf16, mask=None if pre is None else pre > 0), f.grad, "code")
    assert 1e-4 < y["l2"][0] < H.CAP_L2 / H.FACTOR["l2"]


def test_segmenter_refuses_what_dino_depth_cannot_run():
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    with pytest.raises(ValueError, match="aug_alignment_weight"):
        UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance="sum", aug_alignment_weight=0.5))
    for guidance in ("sum", "cross_attn"):
        with pytest.raises(ValueError, match="rec_weight"):
            UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance=guidance, rec_weight=0.5))
    UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance="none", rec_weight=0.5))
    # a configuration changed after construction is refused in front of the step's first launch
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance="sum"))
    seg.cfg.aug_alignment_weight = 0.5
    with pytest.raises(ValueError, match="aug_alignment_weight"):
        seg.training_step({"img": None, "img_pos": None, "label": None, "depth": None, "depth_pos": None})


def test_segmenter_arch_key_selects_the_featurizer():
    from depthg_amd.featurizer import DepthGuidance
    from depthg_amd.segmenter import StandInFeaturizerWithDepth, UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(3)
    base = UnsupervisedSegmenter(5, default_segmenter_cfg())
    cfg = default_segmenter_cfg()
    del cfg.arch
    torch.manual_seed(3)
    absent = UnsupervisedSegmenter(5, cfg)
    assert not isinstance(absent.net, DepthGuidance) and not isinstance(base.net, DepthGuidance)
    assert list(absent.state_dict()) == list(base.state_dict())
    assert not any(k.startswith(("net.depth_downscaling", "net.cross_attn", "net.no_depth_embed")) for k in base.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(absent.state_dict().values(), base.state_dict().values()))
    torch.manual_seed(3)
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance="sum", use_depth=False))
    assert isinstance(seg.net, StandInFeaturizerWithDepth) and seg.use_depth is True
    for k, v in base.net.state_dict().items():                             # the head's initial values are the plain featurizer's
        assert torch.equal(seg.net.state_dict()[k], v), k
    stepped = seg.head_parameters()
    names = {n for n, p in seg.net.named_parameters() if any(p is q for q in stepped)}
    assert names == {n for n, _ in seg.net.named_parameters() if n.split(".")[0] in ("cluster1", "cluster2", "depth_downscaling")}
    assert [id(p) for p in seg.all_reduced_parameters()] == \
        [id(p) for o in seg.configure_optimizers() for grp in o.param_groups for p in grp["params"]]
