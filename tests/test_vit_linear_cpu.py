"""CPU-side checks of the fused linear layers of the ViT (depthg_amd/csrc/dg_linear.hip, ops.vit_linear_pack / vit_linear_forward,
vit.VisionTransformer(fused_linear=...), cfg.dg_fused_linear): the entry points exist, the flag is off by default and changes nothing
when off, the packed weights are a cache and not state, the refusals, and the emulation that carries the GPU tests' criterion."""
import os
import re
import warnings

import pytest
import torch

import attention_reference as AR
import linear_reference as LR
from conftest import ROOT, load_golden

NAMES = {"dg_vit_linear_packed_bytes", "dg_vit_linear_pack", "dg_vit_linear_forward"}


def test_library_declares_the_linear_entry_points():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    assert NAMES <= set(re.findall(r"\b(dg_[a-z_]+)\s*\(", header))
    assert NAMES <= set(_lib.EXPORTS)
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.dg_version() == 119


def test_pack_sizes():
    from depthg_amd import _lib, ops
    lib = _lib.load()
    for K, Nout in [(384, 1152), (1536, 384), (768, 3072), (128, 512)]:
        assert lib.dg_vit_linear_packed_bytes(K, Nout) == 2 * K * Nout
        assert ops.vit_linear_supported(K, Nout)
    for K, Nout in [(100, 384), (384, 0), (0, 384), (384, 100), (3136, 384), (384, 3136), (-64, 64)]:
        assert lib.dg_vit_linear_packed_bytes(K, Nout) == 0
        assert not ops.vit_linear_supported(K, Nout)
    # unsupported sizes are refused before any launch (no GPU is needed to be told so)
    assert lib.dg_vit_linear_forward(None, None, None, 1e-6, None, None, None, None, 10, 100, 384, 0, None) == -2
    assert b"K=100" in lib.dg_last_error()
    assert lib.dg_vit_linear_pack(None, 384, 96, None, None) == -2


def test_flag_off_is_the_default_and_bit_identical():
    from depthg_amd import vit
    from depthg_amd.segmenter import default_segmenter_cfg
    assert default_segmenter_cfg().dg_fused_linear is False
    fx = load_golden("vit.npz")
    a = AR.seed_module(vit.VisionTransformer(**AR.TINY), int(fx["vit_seed"])).eval()
    b = AR.seed_module(vit.VisionTransformer(**AR.TINY, fused_linear=False), int(fx["vit_seed"])).eval()
    assert a.fused_linear is False and b.fused_linear is False
    x = torch.from_numpy(fx["x"])
    with torch.no_grad():
        assert torch.equal(a.forward_feats(x), b.forward_feats(x))
        fa, fb = a.get_intermediate_feat(x, n=2), b.get_intermediate_feat(x, n=2)
        for ta, tb in zip(fa[0] + fa[1] + fa[2], fb[0] + fb[1] + fb[2]):
            assert torch.equal(ta, tb)
        assert torch.equal(a.get_last_selfattention(x), b.get_last_selfattention(x))


@pytest.mark.parametrize("arch,patch", [("vit_small", 8), ("vit_base", 16)])
def test_state_dict_with_the_flag_on_is_a_dino_checkpoints(arch, patch):
    from depthg_amd import vit
    fx = load_golden("vit.npz")
    sd = vit.ARCHS[arch](patch_size=patch, fused_linear=True).state_dict()
    assert [k + ":" + ",".join(str(d) for d in v.shape) for k, v in sd.items()] == [str(s) for s in fx[f"keys_{arch}_{patch}"]]


def _emulated_ops(monkeypatch, counts):
    """ops.vit_linear_pack / vit_linear_forward replaced by torch emulations that run on the CPU and count their calls."""
    from depthg_amd import ops

    def pack(weight):
        counts["pack"] = counts.get("pack", 0) + 1
        return weight.detach().clone()

    def forward(x, packed, n_out, bias=None, *, ln_weight=None, ln_bias=None, eps=1e-6, gelu=False, residual=None, out=None,
                out_bf16=False):
        counts["forward"] = counts.get("forward", 0) + 1
        a = x.float()
        if ln_weight is not None:
            a = torch.nn.functional.layer_norm(a, a.shape[-1:], ln_weight, ln_bias, eps)
        y = torch.nn.functional.linear(LR.bf16(a), LR.bf16(packed), bias)
        if gelu:
            y = torch.nn.functional.gelu(y)
        if residual is not None:
            y = residual + y
        y = y.to(torch.bfloat16) if out_bf16 else y
        return y if out is None else out.copy_(y)

    monkeypatch.setattr(ops, "vit_linear_pack", pack)
    monkeypatch.setattr(ops, "vit_linear_forward", forward)


def test_packed_weights_are_a_cache_that_follows_the_weights(monkeypatch):
    from depthg_amd import vit
    counts = {}
    _emulated_ops(monkeypatch, counts)
    m = AR.seed_module(vit.VisionTransformer(**AR.TINY, fused_linear=True), 3).eval()
    blk = m.blocks[0]
    assert all(blk.pack_is_stale(n) for n in ("qkv", "proj", "fc1", "fc2"))
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    keys = list(m.state_dict().keys())
    with torch.no_grad():
        first = m.forward_feats(x)
        assert counts["pack"] == 8 and counts["forward"] == 8                  # 2 blocks x 4 layers
        assert not any(blk.pack_is_stale(n) for n in ("qkv", "proj", "fc1", "fc2"))
        assert torch.equal(m.forward_feats(x), first) and counts["pack"] == 8    # the cache is hit
        assert list(m.state_dict().keys()) == keys                              # ... and is not state
        assert not any("pack" in k for k in keys)
        # the emulated fused model is the bf16-operand model: the route through the block is the reference's
        exact = AR.seed_module(vit.VisionTransformer(**AR.TINY), 3).eval().forward_feats(x)
        assert 0 < LR.rel_l2(first, exact.double()) < 2e-2
        # load_state_dict: every pack is stale and the output follows the new weights
        AR.seed_module(m, 4)
        assert all(b.pack_is_stale(n) for b in m.blocks for n in ("qkv", "proj", "fc1", "fc2"))
        second = m.forward_feats(x)
        assert counts["pack"] == 16 and not torch.equal(first, second)
        want = AR.seed_module(vit.VisionTransformer(**AR.TINY), 4).eval().forward_feats(x)
        assert LR.rel_l2(second, want.double()) < 2e-2
        # an in-place edit of one weight: that pack alone
        blk.mlp.fc2.weight.mul_(0.5)
        assert blk.pack_is_stale("fc2") and not blk.pack_is_stale("fc1")
        m.forward_feats(x)
        assert counts["pack"] == 17
        # a new storage (what .to(device) leaves behind)
        blk.attn.qkv.weight.data = blk.attn.qkv.weight.data.clone()
        assert blk.pack_is_stale("qkv")


def test_fused_contracts_on_the_emulated_ops(monkeypatch):
    """return_attention / return_qkv / get_intermediate_feat / get_last_selfattention keep their shapes and meanings."""
    from depthg_amd import vit
    _emulated_ops(monkeypatch, {})
    m = AR.seed_module(vit.VisionTransformer(**AR.TINY, fused_linear=True), 3).eval()
    ref = AR.seed_module(vit.VisionTransformer(**AR.TINY), 3).eval()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        x0 = m.prepare_tokens(x)
        keep = x0.clone()
        m.blocks[0](x0, fused_linear=True)
        assert torch.equal(x0, keep), "the block changed its input"
        feat, attn, qkv = m.get_intermediate_feat(x, n=2)
        rfeat, rattn, rqkv = ref.get_intermediate_feat(x, n=2)
        assert len(feat) == len(attn) == len(qkv) == 2
        for got, want in zip(feat + attn + qkv, rfeat + rattn + rqkv):
            assert got.shape == want.shape and LR.rel_l2(got, want.double()) < 2e-2
        last = m.get_last_selfattention(x)
        assert torch.allclose(last.sum(-1), torch.ones_like(last.sum(-1)), atol=1e-5)
        assert LR.rel_l2(last, ref.get_last_selfattention(x).double()) < 2e-2
        assert LR.rel_l2(m(x), ref(x).double()) < 2e-2
        assert LR.rel_l2(m.get_intermediate_layers(x, n=1)[0], ref.get_intermediate_layers(x, n=1)[0].double()) < 2e-2


def test_refusals():
    from depthg_amd import ops, vit
    with pytest.raises(ValueError, match="100"):
        vit.VisionTransformer(img_size=[32], patch_size=8, embed_dim=100, depth=1, num_heads=2, fused_linear=True)
    with pytest.raises(ValueError, match="1024"):
        vit.VisionTransformer(img_size=[32], patch_size=8, embed_dim=1024, depth=1, num_heads=16, mlp_ratio=2., fused_linear=True)
    vit.VisionTransformer(img_size=[32], patch_size=8, embed_dim=100, depth=1, num_heads=2)          # fine without the flag
    # the fused path on CPU tensors: no quiet fall-back to torch
    m = vit.VisionTransformer(**AR.TINY, fused_linear=True).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        m.forward_feats(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vit_linear_pack(torch.zeros(384, 128))
    packed = torch.zeros(2 * 128 * 384, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vit_linear_forward(torch.zeros(10, 128), packed, 384)
    with pytest.raises(RuntimeError, match="no backward"):
        ops.vit_linear_forward(torch.zeros(10, 128, requires_grad=True), packed, 384)
    with pytest.raises(ValueError, match="multiples of 64"):
        ops.vit_linear_forward(torch.zeros(10, 100), packed, 384)
    with pytest.raises(ValueError, match="multiples of 64"):
        ops.vit_linear_pack(torch.zeros(384, 100))
    with pytest.raises(ValueError, match="float32"):
        ops.vit_linear_forward(torch.zeros(10, 128, dtype=torch.float64), packed, 384)
    with pytest.raises(ValueError, match="float32"):
        ops.vit_linear_forward(torch.zeros(10, 128, dtype=torch.bfloat16), packed, 384, ln_weight=torch.ones(128), ln_bias=torch.zeros(128))
    with pytest.raises(ValueError, match="contiguous"):
        ops.vit_linear_forward(torch.zeros(128, 10).t(), packed, 384)
    with pytest.raises(ValueError, match="768"):
        ops.vit_linear_forward(torch.zeros(10, 1536), packed, 384, ln_weight=torch.ones(1536), ln_bias=torch.zeros(1536))
    with pytest.raises(ValueError, match="residual"):
        ops.vit_linear_forward(torch.zeros(10, 128), packed, 384, residual=torch.zeros(10, 384), out_bf16=True)


def test_featurizer_reads_the_cfg_key():
    from depthg_amd import DinoFeaturizer
    from depthg_amd.segmenter import default_segmenter_cfg
    for on in (False, True):
        cfg = default_segmenter_cfg(model_type="vit_small", dino_patch_size=8, dropout=False, dg_dino_vit_kwargs=dict(AR.TINY),
                                    dg_fused_linear=on)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = DinoFeaturizer(70, cfg)
        assert net.model.fused_linear is on and net.model.fused_attention is False


@pytest.mark.parametrize("kind,K", [(kind, K) for kind in LR.KINDS for K in (128, 384, 768, 1536) if LR.kind_fits(kind, K)])
def test_emulation_of_the_prescribed_arithmetic_stays_within_the_factor(kind, K):
    for sigma in (1.0, 3.0):
        case = LR.make_case(kind, 257, K, 384, sigma, seed=K)
        err, yard = LR.ratios(LR.emulate(kind, case), kind, case)
        print(f"emulation {kind} K={K} sigma={sigma}: {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
        assert err <= LR.FACTOR * yard, (err, yard)
        assert err / yard < 1.3                  # the module docstring's table
