"""GPU tests of the fused attention kernel (depthg_amd/csrc/dg_attn.hip k_attn_fwd through ops.attention_forward), of
cfg.dg_fused_attention in the whole ViT, and of featurizer.DinoFeaturizer / cfg.dg_dino_backbone in the segmenter.

The kernel's criterion (tests/attention_reference.py): relative L2 error against the float64 attention <= 1.5 x the error of the
same float64 attention on q, k, v rounded to bf16.  Every case prints its two figures before it asserts (-s shows them;
scripts/vit_parity.py tabulates them into profiles/vit_parity.md).
"""
import numpy as np
import pytest
import torch

import attention_reference as AR
from conftest import load_golden

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 4096                      # floats on either side (a multiple of 4: the tensors stay 16-byte aligned)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _guarded_call(qkv_cpu, heads, scale, dev):
    """ops.attention_forward on an input followed by a NaN guard, into an output between two sentinel guards.  Returns the result
    (a copy) after checking that the guards are untouched."""
    from depthg_amd import ops
    B, N, C3 = qkv_cpu.shape
    n_in, n_out = qkv_cpu.numel(), B * N * C3 // 3
    src = torch.full((n_in + GUARD,), float("nan"), device=dev)
    src[:n_in] = qkv_cpu.reshape(-1).to(dev)
    buf = torch.full((GUARD + n_out + GUARD,), SENTINEL, device=dev)
    out = buf[GUARD:GUARD + n_out].view(B, N, C3 // 3)
    got = ops.attention_forward(src[:n_in].view(B, N, C3), heads, scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n_out:] == SENTINEL).all()), "a guard of the output was written"
    assert bool(torch.isnan(src[n_in:]).all())
    assert bool(torch.isfinite(out).all()), "a value outside the tensor reached the result (or the softmax overflowed)"
    return out.clone()


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [1, 6, 12])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 197, 785, 1601])
def test_kernel_within_factor_of_bf16_operand_error(N, heads, B, sigma, dev):
    qkv = AR.seeded_qkv(B, N, heads, sigma, seed=1000 * N + 10 * heads + B)
    got = _guarded_call(qkv, heads, 0.125, dev)
    err, yard = AR.ratios(got, qkv.to(dev), heads, 0.125)
    print(f"attention N={N} heads={heads} B={B} sigma={sigma}: kernel {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    assert err <= AR.FACTOR * yard, (err, yard)


def test_dominant_score_row(dev):
    """q = 40 k_j: a softmax without the running maximum gives NaN; the expected output is v_j."""
    B, N, heads, j = 2, 197, 6, 77
    qkv = AR.dominant_qkv(B, N, heads, j, seed=5)
    got = _guarded_call(qkv, heads, 0.125, dev)
    err, yard = AR.ratios(got, qkv.to(dev), heads, 0.125)
    print(f"attention dominant row: kernel {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    assert err <= AR.FACTOR * yard, (err, yard)
    v_j = qkv.reshape(B, N, 3, heads * 64)[:, j:j + 1, 2].to(dev).double()
    assert AR.rel_l2(got, v_j.expand(B, N, heads * 64)) <= AR.FACTOR * yard


def test_other_scale_and_default(dev):
    from depthg_amd import ops
    qkv = AR.seeded_qkv(2, 130, 6, 1.0, seed=11).to(dev)
    err, yard = AR.ratios(ops.attention_forward(qkv, 6, scale=0.3), qkv, 6, 0.3)
    assert err <= AR.FACTOR * yard, (err, yard)
    assert torch.equal(ops.attention_forward(qkv, 6), ops.attention_forward(qkv, 6, scale=0.125))


def test_two_calls_bit_identical_and_side_stream(dev):
    from depthg_amd import ops
    qkv = AR.seeded_qkv(3, 785, 6, 1.0, seed=3).to(dev)
    a = ops.attention_forward(qkv, 6)
    b = ops.attention_forward(qkv, 6)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = ops.attention_forward(qkv, 6)
    side.synchronize()
    assert torch.equal(a, c)


def test_refusals_on_the_gpu(dev):
    from depthg_amd import ops
    q = torch.zeros(2, 10, 3 * 6 * 64, device=dev)
    with pytest.raises(ValueError, match="head dimension 64"):
        ops.attention_forward(torch.zeros(2, 10, 3 * 6 * 32, device=dev), 6)
    with pytest.raises(ValueError, match="float32"):
        ops.attention_forward(q.half(), 6)
    with pytest.raises(ValueError, match="contiguous"):
        ops.attention_forward(torch.zeros(10, 2, 3 * 6 * 64, device=dev).transpose(0, 1), 6)
    with pytest.raises(ValueError, match="out"):
        ops.attention_forward(q, 6, out=torch.zeros(2, 10, 6 * 64 + 1, device=dev))


@pytest.mark.parametrize("hw", [(224, 224), (224, 320)])
def test_whole_vit_small_fused_vs_fp32(hw, dev):
    """vit_small(8), seeded random weights (no pretrained checkpoint is available to the tests): final-norm features with the fused
    kernel against the fp32 torch path, bounded by 1.5 x the same model with q, k, v rounded to bf16 in the torch attention."""
    from depthg_amd import vit
    model = AR.seed_module(vit.vit_small(8), 42).to(dev).eval()
    x = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(7)).to(dev)
    with torch.no_grad():
        exact = model.forward_feats(x)
        yard = AR.bf16_operand_model(model).forward_feats(x)
        model.fused_attention = True
        fused = model.forward_feats(x)
    e, y = _rel(fused, exact), _rel(yard, exact)
    print(f"vit_small(8) {hw}: fused {e:.3e} bf16-operand yardstick {y:.3e} ratio {e / y:.3f}")
    assert e <= AR.FACTOR * y, (e, y)


def _tiny_cfg(**over):
    from depthg_amd.segmenter import default_segmenter_cfg
    return default_segmenter_cfg(**{**dict(model_type="vit_small", dino_patch_size=8, dg_dino_backbone=True, feature_samples=5,
                                           dg_dino_vit_kwargs=dict(AR.TINY)), **over})


def _fixture_featurizer(fx, feat_type, dev, **over):
    from depthg_amd import DinoFeaturizer
    arch = AR.TINY if feat_type == "feat" else AR.TINY6
    cfg = _tiny_cfg(dino_feat_type=feat_type, dropout=False, dg_dino_vit_kwargs=dict(arch), **over)
    with pytest.warns(UserWarning, match="pretrained_weights"):
        net = DinoFeaturizer(int(fx["dim"]), cfg)
    AR.seed_module(net.model, int(fx["vit_seed"]), fx["tiny_checksum" if feat_type == "feat" else "tiny6_checksum"])
    head = torch.nn.Module()
    head.cluster1, head.cluster2 = net.cluster1, net.cluster2
    AR.seed_module(head, int(fx["head_seed"]), fx[f"dino_{feat_type}_head_checksum"])
    return net.to(dev)


@pytest.mark.parametrize("feat_type", ["feat", "KK"])
def test_dino_featurizer_reproduces_reference_outputs(feat_type, dev):
    """flag off: feats 1e-5 relative, code to the tolerance of tests/test_gpu_head.py (the head is bf16 MFMA)."""
    fx = load_golden("vit.npz")
    net = _fixture_featurizer(fx, feat_type, dev).eval()
    x = torch.from_numpy(fx["x"]).to(dev)
    feats, code = net(x)
    want_f, want_c = torch.from_numpy(fx[f"dino_{feat_type}_feats"]), torch.from_numpy(fx[f"dino_{feat_type}_code"])
    print(f"DinoFeaturizer {feat_type}: feats {_rel(feats.cpu(), want_f):.3e} code {_rel(code.cpu(), want_c):.3e}")
    assert _rel(feats.cpu(), want_f) < 1e-5
    assert (code.cpu() - want_c).abs().max() < 1.5e-2 * want_c.abs().max() and _rel(code.cpu(), want_c) < 6e-3
    cls = net(x, return_class_feat=True)
    assert _rel(cls.cpu(), torch.from_numpy(fx[f"dino_{feat_type}_class"])) < 1e-5
    # the fused kernel on the same backbone: bf16-operand error only
    fused = _fixture_featurizer(fx, feat_type, dev, dg_fused_attention=True).eval()
    feats_f, _ = fused(x)
    if feat_type == "feat":
        assert 0 < _rel(feats_f.cpu(), want_f) < 2e-2
    else:                       # the last block's keys do not pass through an attention at depth 1
        assert _rel(feats_f.cpu(), want_f) < 1e-5


def _batch(dev, B=2, hw=40, n_classes=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
            "label": torch.randint(0, n_classes, (B, hw, hw), generator=g).to(dev),
            "depth": torch.rand(B, 1, hw, hw, generator=g).to(dev), "depth_pos": torch.rand(B, 1, hw, hw, generator=g).to(dev)}


@pytest.mark.parametrize("fused", [False, True])
def test_segmenter_with_dino_backbone(fused, dev):
    from depthg_amd import DinoFeaturizer
    from depthg_amd.segmenter import UnsupervisedSegmenter
    with pytest.warns(UserWarning, match="pretrained_weights"):
        seg = UnsupervisedSegmenter(5, _tiny_cfg(dg_fused_attention=fused)).to(dev)
    assert isinstance(seg.net, DinoFeaturizer) and seg.net.model.fused_attention is fused
    seg.train()
    batch = _batch(dev)
    loss, logs = seg.training_step(batch, 0)
    assert bool(torch.isfinite(loss))
    with_grad = {n for n, p in seg.net.named_parameters() if p.grad is not None and float(p.grad.abs().sum()) > 0}
    assert with_grad == {n for n, _ in seg.net.named_parameters() if n.startswith(("cluster1.", "cluster2."))}
    assert all(p.grad is None for p in seg.net.model.parameters())
    out = seg.validation_step(batch, 0)
    assert out["linear_preds"].shape[-2:] == batch["label"].shape[-2:]
    lin, clu = seg.evaluate_batch(batch)
    assert lin.shape == batch["label"].shape and clu.shape == batch["label"].shape
    assert seg.net.training                                   # the mode is restored for the next training_step


@pytest.mark.parametrize("fused", [False, True])
def test_lhp_attn_strategy_receives_the_real_attention(fused, dev, monkeypatch):
    from depthg_amd.segmenter import UnsupervisedSegmenter
    cfg = _tiny_cfg(dg_fused_attention=fused, lhp=True, propagation_strategy="attn")
    with pytest.warns(UserWarning, match="pretrained_weights"):
        seg = UnsupervisedSegmenter(5, cfg).to(dev)
    seg.train()
    seen = []
    real = seg.lhp_module.forward
    monkeypatch.setattr(seg.lhp_module, "forward", lambda code, depth, img=None, attn=None: (seen.append(attn), real(code, depth, img, attn))[1])
    loss, _ = seg.training_step(_batch(dev), 0)
    assert bool(torch.isfinite(loss))
    attn = next(a for a in seen if a is not None)
    assert tuple(attn.shape) == (2, 2, 26, 26)
    assert torch.allclose(attn.sum(-1), torch.ones_like(attn.sum(-1)), atol=1e-5)
    if fused:                 # block 0 ran fused, the last block in fp32: close to the fp32 model's attention, not equal
        seg.net.model.fused_attention = False
        exact = seg.net.model.get_last_selfattention(_batch(dev)["img"])
        assert 0 < _rel(attn, exact) < 2e-2
