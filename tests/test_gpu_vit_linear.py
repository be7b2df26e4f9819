"""GPU tests of the fused linear kernel (depthg_amd/csrc/dg_linear.hip k_lin_fwd through ops.vit_linear_forward), of
cfg.dg_fused_linear in the whole ViT, and of the flag in featurizer.DinoFeaturizer / the segmenter.

The kernel's criterion (tests/linear_reference.py): relative L2 error against the float64 layer <= 1.5 x the error of the same
float64 layer with the A operand and the weight rounded to bf16.  Every case prints its two figures before it asserts (-s shows
them; scripts/vit_parity.py tabulates them into profiles/vit_linear_parity.md).
"""
import pytest
import torch

import attention_reference as AR
import linear_reference as LR

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 4096                      # elements on either side (a multiple of 8: the tensors stay 16-byte aligned)
SHAPES = [(128, 384), (384, 1152), (384, 384), (384, 1536), (1536, 384), (768, 2304), (3072, 768)]
MS = [1, 63, 64, 129, 785, 3 * 1601]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def run_kernel(kind, case, dev, alias=False, packed=None):
    """ops.vit_linear_forward of one case: the input followed by a NaN guard, the output between two sentinel guards and pre-filled
    with NaN.  alias: the output buffer holds the residual and is passed as both.  Returns the result (a copy)."""
    from depthg_amd import ops
    ln, gelu, res, in_bf16, out_bf16 = LR.KINDS[kind]
    x = case["x"]
    M, K = x.shape
    Nout = case["w"].shape[0]
    src = torch.full((M * K + GUARD,), float("nan"), device=dev, dtype=x.dtype)
    src[:M * K] = x.reshape(-1).to(dev)
    odt = torch.bfloat16 if out_bf16 else torch.float32
    buf = torch.full((GUARD + M * Nout + GUARD,), SENTINEL, device=dev, dtype=odt)
    out = buf[GUARD:GUARD + M * Nout].view(M, Nout)
    out.fill_(float("nan"))
    g = {k: (v.to(dev) if v is not None else None) for k, v in case.items()}
    residual = g["residual"]
    if alias:
        out.copy_(residual)
        residual = out
    if packed is None:
        packed = ops.vit_linear_pack(g["w"])
    got = ops.vit_linear_forward(src[:M * K].view(M, K), packed, Nout, g["b"], ln_weight=g["gamma"], ln_bias=g["beta"], eps=LR.EPS,
                                 gelu=gelu, residual=residual, out=out, out_bf16=out_bf16)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + M * Nout:] == SENTINEL).all()), "a guard of the output was written"
    assert bool(torch.isnan(src[M * K:]).all())
    assert bool(torch.isfinite(out.float()).all()), "an element was left unwritten, or a value outside the tensors reached the result"
    return out.clone()


def _on(case, dev):
    return {k: (v.to(dev) if v is not None else None) for k, v in case.items()}


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K,Nout", SHAPES)
@pytest.mark.parametrize("kind", list(LR.KINDS))
def test_kernel_within_factor_of_bf16_operand_error(kind, K, Nout, M, dev):
    if not LR.kind_fits(kind, K):
        with pytest.raises(ValueError, match="768"):           # the case does not exist: the LayerNorm prologue ends at K = 768
            from depthg_amd import ops
            ops.vit_linear_forward(torch.zeros(M, K, device=dev), torch.zeros(2 * K * Nout, dtype=torch.uint8, device=dev), Nout,
                                   ln_weight=torch.ones(K, device=dev), ln_bias=torch.zeros(K, device=dev))
        return
    for sigma in (1.0, 3.0):
        case = LR.make_case(kind, M, K, Nout, sigma, seed=100 * K + Nout + M)
        got = run_kernel(kind, case, dev)
        err, yard = LR.ratios(got, kind, _on(case, dev))
        print(f"linear {kind} K={K} Nout={Nout} M={M} sigma={sigma}: kernel {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
        assert err <= LR.FACTOR * yard, (err, yard)


def test_large_common_offset_rows(dev):
    """Rows of 100 + randn alone: a one-pass E[x^2] - mean^2 variance in fp32 is off by 1e-2 relative here."""
    case = LR.make_case("ln", 64, 384, 384, 1.0, seed=9)
    g = torch.Generator().manual_seed(10)
    case["x"] = 100.0 + torch.randn(64, 384, generator=g)
    got = run_kernel("ln", case, dev)
    err, yard = LR.ratios(got, "ln", _on(case, dev))
    print(f"linear ln offset rows: kernel {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    assert err <= LR.FACTOR * yard, (err, yard)


def test_no_bias_and_leading_dims(dev):
    from depthg_amd import ops
    case = LR.make_case("res", 2 * 197, 384, 384, 1.0, seed=21)
    c = _on(case, dev)
    packed = ops.vit_linear_pack(c["w"])
    flat = ops.vit_linear_forward(c["x"], packed, 384, None, residual=c["residual"])
    shaped = ops.vit_linear_forward(c["x"].view(2, 197, 384), packed, 384, None, residual=c["residual"].view(2, 197, 384))
    assert tuple(shaped.shape) == (2, 197, 384) and torch.equal(shaped.view(-1, 384), flat)
    c["b"] = torch.zeros_like(c["b"])
    err, yard = LR.ratios(flat, "res", c)
    assert err <= LR.FACTOR * yard, (err, yard)


@pytest.mark.parametrize("kind", ["res", "bf16_res"])
def test_out_aliased_to_residual(kind, dev):
    case = LR.make_case(kind, 785, 1536 if kind == "bf16_res" else 384, 384, 1.0, seed=31)
    assert torch.equal(run_kernel(kind, case, dev), run_kernel(kind, case, dev, alias=True))


def test_two_calls_bit_identical_and_side_stream(dev):
    from depthg_amd import ops
    case = LR.make_case("ln_gelu_bf16", 3 * 785, 384, 1536, 1.0, seed=41)
    c = _on(case, dev)
    packed = ops.vit_linear_pack(c["w"])
    kw = dict(ln_weight=c["gamma"], ln_bias=c["beta"], gelu=True, out_bf16=True)
    a = ops.vit_linear_forward(c["x"], packed, 1536, c["b"], **kw)
    b = ops.vit_linear_forward(c["x"], packed, 1536, c["b"], **kw)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s = ops.vit_linear_forward(c["x"], ops.vit_linear_pack(c["w"]), 1536, c["b"], **kw)
    side.synchronize()
    assert torch.equal(a, s)
    err, yard = LR.ratios(s, "ln_gelu_bf16", c)
    assert err <= LR.FACTOR * yard, (err, yard)


def test_poisoned_buffers(dev, monkeypatch):
    """DG_POISON semantics: the buffers ops hands out are pre-filled with 0xFF bytes (NaN); nothing of them is left unwritten."""
    from depthg_amd import ops
    monkeypatch.setattr(ops, "POISON", True)
    for kind in LR.KINDS:
        case = LR.make_case(kind, 129, 384, 384, 1.0, seed=51)
        c = _on(case, dev)
        ln, gelu, res, in_bf16, out_bf16 = LR.KINDS[kind]
        packed = ops.vit_linear_pack(c["w"])
        got = ops.vit_linear_forward(c["x"], packed, 384, c["b"], ln_weight=c["gamma"], ln_bias=c["beta"], gelu=gelu,
                                     residual=c["residual"], out_bf16=out_bf16)
        assert bool(torch.isfinite(got.float()).all())
        err, yard = LR.ratios(got, kind, c)
        assert err <= LR.FACTOR * yard, (kind, err, yard)


def test_refusals_on_the_gpu(dev):
    from depthg_amd import _lib, ops
    x = torch.zeros(10, 384, device=dev)
    packed = ops.vit_linear_pack(torch.zeros(384, 384, device=dev))
    with pytest.raises(ValueError, match="aligned"):
        ops.vit_linear_forward(torch.zeros(10 * 384 + 1, device=dev)[1:].view(10, 384), packed, 384)
    with pytest.raises(ValueError, match="aligned"):
        ops.vit_linear_forward(x, packed, 384, out=torch.zeros(10 * 384 + 2, device=dev)[2:].view(10, 384))
    with pytest.raises(ValueError, match="multiples of 64"):
        ops.vit_linear_forward(torch.zeros(10, 100, device=dev), packed, 384)
    with pytest.raises(ValueError, match="multiples of 64"):
        ops.vit_linear_pack(torch.zeros(96, 384, device=dev))
    with pytest.raises(ValueError, match="float32"):
        ops.vit_linear_forward(x.half(), packed, 384)
    with pytest.raises(ValueError, match="float32"):
        ops.vit_linear_pack(torch.zeros(384, 384, device=dev, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="out"):
        ops.vit_linear_forward(x, packed, 384, out=torch.zeros(10, 384, device=dev, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="packed"):
        ops.vit_linear_forward(x, packed[:-16], 384)
    with pytest.raises(ValueError, match="alias"):
        ops.vit_linear_forward(x, packed, 384, out=x)
    with pytest.raises(RuntimeError, match="no backward"):
        ops.vit_linear_forward(torch.zeros(10, 384, device=dev, requires_grad=True), packed, 384)
    # the C ABI itself: a misaligned pointer and an unsupported width, before any launch
    lib = _lib.load()
    rc = lib.dg_vit_linear_forward(x.data_ptr() + 4, None, None, 1e-6, packed.data_ptr(), None, None, torch.zeros(10, 384, device=dev).data_ptr(),
                                   9, 384, 384, 0, None)
    assert rc == -1 and b"aligned" in lib.dg_last_error()
    assert lib.dg_vit_linear_forward(x.data_ptr(), None, None, 1e-6, packed.data_ptr(), None, None, x.data_ptr(), 10, 96, 384, 0, None) == -2


FLAGS = [(False, True), (True, True), (True, False), (False, False)]          # (fused_attention, fused_linear)


@pytest.mark.parametrize("hw", [(224, 224), (224, 320)])
def test_whole_vit_small_fused_vs_fp32(hw, dev):
    """vit_small(8), seeded random weights (no pretrained checkpoint is available to the tests), all four flag combinations: the
    error against the fp32 torch model is bounded by 1.5 x the error of the torch model that rounds the same operands to bf16."""
    from depthg_amd import vit
    model = AR.seed_module(vit.vit_small(8), 42).to(dev).eval()
    x = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(7)).to(dev)

    def outputs(m):
        feat, _, qkv = m.get_intermediate_feat(x, n=1, want_attn=False)
        B, N = feat[0].shape[:2]
        kk = qkv[0][1].permute(0, 2, 1, 3).reshape(B, N, -1)             # "KK": the last block's keys (src/modules.py:112-114)
        return {"forward_feats": m.forward_feats(x), "feat": feat[0], "KK": kk}

    with torch.no_grad():
        exact = outputs(model)
        for fa, fl in FLAGS:
            if not (fa or fl):
                again = outputs(model)
                assert all(torch.equal(again[k], exact[k]) for k in exact)           # flags off: the fp32 torch path, bit for bit
                continue
            yard = outputs(LR.bf16_operand_model(model, linear=fl, attention=fa))
            model.fused_attention, model.fused_linear = fa, fl
            fused = outputs(model)
            model.fused_attention = model.fused_linear = False
            for name in exact:
                e, y = _rel(fused[name], exact[name]), _rel(yard[name], exact[name])
                print(f"vit_small(8) {hw} attention={fa} linear={fl} {name}: fused {e:.3e} bf16-operand yardstick {y:.3e} ratio {e / y:.3f}")
                assert e <= LR.FACTOR * y, (name, fa, fl, e, y)


def _tiny_cfg(**over):
    from depthg_amd.segmenter import default_segmenter_cfg
    return default_segmenter_cfg(**{**dict(model_type="vit_small", dino_patch_size=8, dg_dino_backbone=True, feature_samples=5,
                                           dg_dino_vit_kwargs=dict(AR.TINY)), **over})


def _batch(dev, B=2, hw=40, n_classes=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
            "label": torch.randint(0, n_classes, (B, hw, hw), generator=g).to(dev),
            "depth": torch.rand(B, 1, hw, hw, generator=g).to(dev), "depth_pos": torch.rand(B, 1, hw, hw, generator=g).to(dev)}


@pytest.mark.parametrize("feat_type", ["feat", "KK"])
@pytest.mark.parametrize("fused_attention", [False, True])
def test_featurizer_and_segmenter_with_fused_linear(fused_attention, feat_type, dev):
    from depthg_amd import DinoFeaturizer
    from depthg_amd.segmenter import UnsupervisedSegmenter
    arch = AR.TINY if feat_type == "feat" else AR.TINY6
    cfg = _tiny_cfg(dg_fused_linear=True, dg_fused_attention=fused_attention, dino_feat_type=feat_type, dg_dino_vit_kwargs=dict(arch))
    with pytest.warns(UserWarning, match="pretrained_weights"):
        seg = UnsupervisedSegmenter(5, cfg).to(dev)
    assert isinstance(seg.net, DinoFeaturizer) and seg.net.model.fused_linear is True
    assert seg.net.model.fused_attention is fused_attention
    before = {n: p.detach().clone() for n, p in seg.net.model.named_parameters()}
    seg.train()
    batch = _batch(dev)
    loss, _ = seg.training_step(batch, 0)
    assert bool(torch.isfinite(loss))
    assert all(p.grad is None for p in seg.net.model.parameters())
    out = seg.validation_step(batch, 0)
    assert out["linear_preds"].shape[-2:] == batch["label"].shape[-2:]
    assert all(bool(torch.isfinite(v).all()) for v in out.values() if isinstance(v, torch.Tensor) and v.is_floating_point())
    assert all(torch.equal(p, before[n]) for n, p in seg.net.model.named_parameters()), "the frozen backbone moved"
    # the features are the fp32 backbone's up to the bf16 operands
    seg.eval()
    with torch.no_grad():
        feats_fused, _ = seg.net(batch["img"])
        seg.net.model.fused_linear = seg.net.model.fused_attention = False
        feats_exact, _ = seg.net(batch["img"])
    assert 0 < _rel(feats_fused, feats_exact) < 3e-2


def test_lhp_attn_strategy_receives_the_real_attention(dev, monkeypatch):
    from depthg_amd.segmenter import UnsupervisedSegmenter
    cfg = _tiny_cfg(dg_fused_linear=True, dg_fused_attention=True, lhp=True, propagation_strategy="attn")
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
    seg.net.model.fused_attention = seg.net.model.fused_linear = False
    exact = seg.net.model.get_last_selfattention(_batch(dev)["img"])
    assert 0 < _rel(attn, exact) < 2e-2


def test_weight_reload_repacks(dev):
    from depthg_amd import vit
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(dev)
    m = AR.seed_module(vit.VisionTransformer(**AR.TINY, fused_linear=True), 5).to(dev).eval()
    ref = vit.VisionTransformer(**AR.TINY).to(dev).eval()
    with torch.no_grad():
        first = m.forward_feats(x)
        assert _rel(first, AR.seed_module(ref, 5).forward_feats(x)) < 2e-2
        AR.seed_module(m, 6)                                               # load_state_dict: different weights, the same storage
        second = m.forward_feats(x)
        want = AR.seed_module(ref, 6).forward_feats(x)
        assert _rel(second, want) < 2e-2 and _rel(first, want) > 0.1, "the fused model kept a stale pack"
        m = m.cpu().to(dev)                                                # new storage
        assert all(b.pack_is_stale(n) for b in m.blocks for n in ("qkv", "proj", "fc1", "fc2"))
        assert torch.equal(m.forward_feats(x), second)
