"""The fused depth encoder (dg_depth_enc.hip) on the GPU: parity with the float64 truth against the bf16 yardstick
(tests/depth_encoder_reference.py: kernel error <= 1.5 x yardstick error, per tensor, L2 and largest element), determinism, the
0xFF pre-fill, the residual, and the featurizer / training step with cfg.dg_fused_depth_encoder."""
import warnings

import pytest
import torch

from tests import depth_encoder_reference as R

pytestmark = pytest.mark.gpu

DEPTH_TOPS = ("depth_downscaling", "cross_attn", "no_depth_embed")
TRAINED = {"sum": ("depth_downscaling",), "cross_attn": ("depth_downscaling", "cross_attn")}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def _inputs(B, h, w, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 1, 8 * h, 8 * w, generator=g), torch.randn(B, C, h, w, generator=g)


def _run(stack, depth, gout, dev, residual=None):
    """(out, ten gradients) of the fused route, twice: the second call's bits must equal the first's."""
    from depthg_amd import depth_encoder
    s = stack.to(dev)
    runs = []
    for _ in range(2):
        s.zero_grad()
        out = depth_encoder(depth.to(dev), s, None if residual is None else residual.to(dev))
        out.backward(gout.to(dev))
        runs.append((out.detach().clone(), [p.grad.clone() for p in R.stack_params(s)]))
    (o1, g1), (o2, g2) = runs
    assert torch.equal(o1, o2), "two forwards differ"
    for name, a, b in zip(R.NAMES, g1, g2):
        assert torch.equal(a, b), f"two backwards differ in d {name}"
    return o1, g1


def _parity(stack, depth, gout, dev, tag):
    out_t, grads_t = R.truth(stack, depth, gout)
    out_y, grads_y = R.yardstick(R.stack_params(stack), depth, gout)
    out, grads = _run(stack, depth, gout, dev)
    R.check(f"{tag} out", out, out_t, out_y)
    for name, g, t, y in zip(R.NAMES, grads, grads_t, grads_y):
        assert g.shape == t.shape
        R.check(f"{tag} d {name}", g, t, y)
    return out, grads


CASES = [(1, 1, 1, 64), (3, 3, 5, 128), (2, 9, 7, 384), (5, 12, 12, 384), (2, 4, 4, 768)]


@pytest.mark.parametrize("B,h,w,C", CASES)
def test_parity(B, h, w, C, dev):
    depth, gout = _inputs(B, h, w, C, 10 + C + B)
    _parity(R.make_stack(C, 20 + B), depth, gout, dev, f"({B},{h}x{w},{C})")


def test_zero_depth(dev):
    depth, gout = _inputs(2, 3, 3, 384, 31)
    _, grads = _parity(R.make_stack(384, 32), torch.zeros_like(depth), gout, dev, "zero depth")
    assert not bool(grads[0].any())                          # d W1 = sum d a1 x depth


def test_zero_variance_in_stage_one(dev):
    stack = R.make_stack(384, 33)
    with torch.no_grad():
        stack[0].weight.zero_()
        stack[0].bias.fill_(0.5)
    depth, gout = _inputs(2, 3, 3, 384, 34)
    out, grads = _parity(stack, depth, gout, dev, "W1 = 0")
    assert all(bool(torch.isfinite(t).all()) for t in (out, *grads))


def test_strided_three_dimensional_depth(dev):
    stack = R.make_stack(128, 35)
    depth, gout = _inputs(2, 2, 3, 128, 36)
    wide = torch.rand(2, 16, 48, generator=torch.Generator().manual_seed(37))
    strided = wide[:, :, ::2]                                 # (B, 8h, 8w), not contiguous
    assert not strided.is_contiguous() and strided.shape == (2, 16, 24)
    out_s, grads_s = _run(stack, strided, gout, dev)
    out_c, grads_c = _run(stack, strided.contiguous().unsqueeze(1), gout, dev)
    assert torch.equal(out_s, out_c) and all(torch.equal(a, b) for a, b in zip(grads_s, grads_c))
    out_t, _ = R.truth(stack, strided, gout)
    out_y, _ = R.yardstick(R.stack_params(stack), strided, gout)
    R.check("strided out", out_s, out_t, out_y)


def test_residual(dev):
    stack = R.make_stack(384, 38)
    depth, gout = _inputs(2, 3, 5, 384, 39)
    res = torch.randn(2, 384, 3, 5, generator=torch.Generator().manual_seed(40))
    out, grads = _run(stack, depth, gout, dev)
    out_r, grads_r = _run(stack, depth, gout, dev, residual=res)
    want = res.to(dev) + out
    spacing = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
    assert bool(((out_r - want).abs() <= spacing).all())
    assert torch.equal(out_r, want)                          # (in fact the same fp32 addition)
    for name, a, b in zip(R.NAMES, grads, grads_r):
        assert torch.equal(a, b), name


def test_poisoned_buffers(dev, monkeypatch):
    """Workspace and outputs pre-filled with 0xFF (the suite's DG_POISON convention): no NaN comes out, same bits as without."""
    from depthg_amd import ops
    stack = R.make_stack(384, 41)
    depth, gout = _inputs(5, 12, 12, 384, 42)
    clean = _run(stack, depth, gout, dev)
    monkeypatch.setattr(ops, "POISON", True)
    out, grads = _run(stack, depth, gout, dev)
    assert all(bool(torch.isfinite(t).all()) for t in (out, *grads))
    assert torch.equal(out, clean[0]) and all(torch.equal(a, b) for a, b in zip(grads, clean[1]))
    o1, g1 = _run(R.make_stack(64, 43), *_inputs(1, 1, 1, 64, 44), dev)
    assert all(bool(torch.isfinite(t).all()) for t in (o1, *g1))


def test_gpu_refusals(dev):
    from depthg_amd import depth_encoder
    stack = R.make_stack(384, 45).to(dev)
    with pytest.raises(ValueError, match="float32"):
        depth_encoder(torch.rand(1, 1, 8, 8, device=dev, dtype=torch.float64), stack)
    with pytest.raises(RuntimeError, match="GPU"):
        depth_encoder(torch.rand(1, 1, 8, 8), stack)
    with pytest.raises(RuntimeError, match="no gradient"):
        depth_encoder(torch.rand(1, 1, 8, 8, device=dev), stack, torch.zeros(1, 384, 1, 1, device=dev, requires_grad=True))


# ---- module level (the shapes and tolerances of tests/test_gpu_depth_featurizer.py)
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


def _tiny_net(dev, guidance, fused):
    from depthg_amd.featurizer import DinoFeaturizerWithDepth
    from depthg_amd.segmenter import default_segmenter_cfg
    cfg = default_segmenter_cfg(dg_dino_vit_kwargs=dict(embed_dim=384, depth=1), dim=16, arch="dino_depth", guidance=guidance,
                                dg_fused_depth_encoder=fused)
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DinoFeaturizerWithDepth(cfg.dim, cfg).to(dev).train()


@pytest.mark.parametrize("guidance", ["sum", "cross_attn"])
def test_featurizer_flag_on_against_flag_off(guidance, dev):
    from depthg_amd.head import draw_keep_masks
    g = torch.Generator().manual_seed(5)
    img, depth = torch.randn(3, 3, 32, 32, generator=g).to(dev), torch.rand(3, 1, 32, 32, generator=g).to(dev)
    up = torch.randn(3, 16, 4, 4, generator=torch.Generator().manual_seed(6)).to(dev)
    torch.manual_seed(4)
    keeps = draw_keep_masks(3, 384, dev)
    res = {}
    for fused in (False, True):
        net = _tiny_net(dev, guidance, fused)
        torch.manual_seed(8)                                   # cross_attn's own dropout draws match
        feats, code, image_feat, attn = net((img, depth), keeps=keeps)
        (code * up).sum().backward()
        res[fused] = (code.detach(), {n: p.grad for n, p in net.named_parameters() if n.split(".")[0] in DEPTH_TOPS})
    code_off, code_on = res[False][0], res[True][0]
    print(f"{guidance} code: L2 {_rel(code_on, code_off):.3e}")
    assert _rel(code_on, code_off) < 6e-3
    seen = 0
    for name, g_off in res[False][1].items():
        g_on = res[True][1][name]
        if name.split(".")[0] in TRAINED[guidance]:
            assert g_on is not None and bool(torch.isfinite(g_on).all()) and g_on.shape == g_off.shape, name
            print(f"{guidance} d {name}: L2 {_rel(g_on, g_off):.3e}")
            assert _rel(g_on, g_off) < 6e-2, (name, _rel(g_on, g_off))
            seen += 1
        else:
            assert g_on is None and g_off is None, name
    assert seen == (10 if guidance == "sum" else 14)


@pytest.mark.parametrize("fused_adam", [False, True])
@pytest.mark.parametrize("guidance", ["sum", "cross_attn"])
def test_training_step_with_the_flag(guidance, fused_adam, dev):
    from depthg_amd.segmenter import StandInFeaturizerWithDepth, UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(11)
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance=guidance, dg_fused_adam=fused_adam, feature_samples=5,
                                                         dg_fused_depth_encoder=True)).to(dev).train()
    assert isinstance(seg.net, StandInFeaturizerWithDepth) and seg.net.fused_depth_encoder
    g = torch.Generator().manual_seed(0)
    batch = {"img": torch.randn(4, 3, 40, 40, generator=g).to(dev), "img_pos": torch.randn(4, 3, 40, 40, generator=g).to(dev),
             "label": torch.randint(0, 5, (4, 40, 40), generator=g).to(dev),
             "depth": torch.rand(4, 1, 40, 40, generator=g).to(dev), "depth_pos": torch.rand(4, 1, 40, 40, generator=g).to(dev)}
    before = {n: p.detach().clone() for n, p in seg.net.named_parameters()}
    loss, logs = seg.training_step(batch)
    assert bool(torch.isfinite(loss))
    stepped = {id(p) for o in seg.optimizers() for grp in o.param_groups for p in grp["params"]}
    assert [id(p) for p in seg.all_reduced_parameters()] == [id(p) for o in seg.optimizers() for grp in o.param_groups for p in grp["params"]]
    moved = 0
    for n, p in seg.net.named_parameters():
        top = n.split(".")[0]
        if top in DEPTH_TOPS:
            trained = top in TRAINED[guidance]
            assert p.requires_grad == trained and (id(p) in stepped) == trained, n
            assert torch.equal(p, before[n]) != trained, (guidance, n)
            moved += trained
    assert moved >= 10
