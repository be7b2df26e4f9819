"""DinoFeaturizerWithDepth (cfg.arch "dino_depth") on the GPU: a tiny ViT (embed_dim 384, one block), 32 x 32 images and depth maps
(a 4 x 4 feature grid), B = 3, dim = 16.  Guidance "none" is DinoFeaturizer bit for bit; "sum" and "cross_attn" are held against a
plain-torch float64 restatement of forward_with_depth (src/modules.py:532-605) with the same keep masks - code and the gradient of
every trainable depth parameter, which reaches it through the head's d image_feat launch - with the tolerances tests/test_gpu_head.py
holds for the head on random inputs (code: 1.5e-2 of the largest element and 6e-3 in L2; a gradient behind cluster2's ReLU mask:
6e-2 in L2 - every depth parameter's gradient passes that mask).  Then one training_step per guidance on the stand-in backbone,
with and without the fused Adam, and the unchanged default step.

test_default_step_is_unchanged pins the loss of one training_step with the `arch` key absent (seed 11, B = 4, 40 x 40 images,
feature_samples = 5, stand-in backbone) as the commit before this feature computed it on an MI355X: 0x1.76d7140000000p+0 (PINNED_LOSS)."""
import copy
import warnings

import pytest
import torch

from oracle import head_oracle as HO

pytestmark = pytest.mark.gpu
PINNED_LOSS = "0x1.76d7140000000p+0"
DEPTH_TOPS = ("depth_downscaling", "cross_attn", "no_depth_embed")
TRAINED = {"none": (), "concat": (), "sum": ("depth_downscaling",), "cross_attn": ("depth_downscaling", "cross_attn")}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


def tiny_cfg(**over):
    from depthg_amd.segmenter import default_segmenter_cfg
    return default_segmenter_cfg(dg_dino_vit_kwargs=dict(embed_dim=384, depth=1), dim=16, **over)


def build(cls, cfg, dev, seed=0):
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cls(cfg.dim, cfg).to(dev)


def inputs(dev, B=3, hw=32, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, hw, hw, generator=g).to(dev), torch.rand(B, 1, hw, hw, generator=g).to(dev)


def restate(net, image_feat, depth, keeps, training):
    """forward_with_depth behind the backbone in float64 on the CPU -> (code, the float64 copies of the depth modules by name)"""
    dd = copy.deepcopy(net.depth_downscaling).double().cpu()
    ca = copy.deepcopy(net.cross_attn).double().cpu().train(training)
    emb = copy.deepcopy(net.no_depth_embed).double().cpu()
    f = image_feat.detach().double().cpu()
    B, C, h, w = f.shape
    kv = f.reshape(B, C, -1).permute(2, 0, 1)
    if training and net.guidance == "sum":
        x = f + dd(depth.double().cpu())
    elif training and net.guidance == "cross_attn":
        x = ca(dd(depth.double().cpu()).reshape(B, C, -1).permute(2, 0, 1), kv, kv)[0].permute(1, 2, 0).reshape(B, C, h, w)
    elif net.guidance == "cross_attn":
        x = ca(emb.weight.reshape(1, 1, -1).expand(h * w, B, -1), kv, kv)[0].permute(1, 2, 0).reshape(B, C, h, w)
    else:
        x = f
    prm = [p.detach().double().cpu() for m in (net.cluster1, net.cluster2) for p in m.parameters()]
    code, _ = HO.head_forward(x, *prm, keeps=None if keeps is None else tuple(k.double().cpu() for k in keeps), p=0.1)
    return code, {"depth_downscaling": dd, "cross_attn": ca, "no_depth_embed": emb}


def test_guidance_none_is_dino_featurizer_bit_for_bit(dev):
    from depthg_amd.featurizer import DinoFeaturizer, DinoFeaturizerWithDepth
    plain = build(DinoFeaturizer, tiny_cfg(), dev).train()
    net = build(DinoFeaturizerWithDepth, tiny_cfg(arch="dino_depth", guidance="none"), dev).train()
    assert net.load_state_dict(plain.state_dict(), strict=False).unexpected_keys == []
    img, depth = inputs(dev)
    torch.manual_seed(9)
    feats_p, code_p, _ = plain(img)
    torch.manual_seed(9)
    out = net((img, depth))
    assert len(out) == 4
    assert torch.equal(out[0], feats_p) and torch.equal(out[1], code_p)
    out[1].square().sum().backward()
    code_p.square().sum().backward()
    for name, p in net.named_parameters():
        if name.split(".")[0] in DEPTH_TOPS:
            assert p.grad is None and not p.requires_grad, name
    for (name, p), q in zip(plain.named_parameters(), [dict(net.named_parameters())[n] for n, _ in plain.named_parameters()]):
        if p.requires_grad:
            assert torch.equal(p.grad, q.grad), name


@pytest.mark.parametrize("guidance", ["sum", "cross_attn"])
def test_training_pass_against_float64_restatement(guidance, dev):
    from depthg_amd.featurizer import DinoFeaturizerWithDepth
    from depthg_amd.head import draw_keep_masks
    net = build(DinoFeaturizerWithDepth, tiny_cfg(arch="dino_depth", guidance=guidance), dev).train()
    net.cross_attn.dropout = 0.0                               # (its mask is torch's own draw: not part of the comparison)
    img, depth = inputs(dev)
    torch.manual_seed(4)
    keeps = draw_keep_masks(3, 384, dev)
    up = torch.randn(3, 16, 4, 4, generator=torch.Generator().manual_seed(6))
    feats, code, image_feat, attn = net((img, depth), keeps=keeps)
    assert code.shape == (3, 16, 4, 4) and feats.shape == image_feat.shape == (3, 384, 4, 4) and not feats.requires_grad
    (code * up.to(dev)).sum().backward()
    want, mods = restate(net, image_feat, depth, keeps, True)
    (want * up.double()).sum().backward()
    print(f"{guidance} code: worst element {float((code.detach().cpu() - want).abs().max() / want.abs().max()):.3e} L2 {_rel(code.detach(), want.detach()):.3e}")
    assert (code.detach().cpu() - want).abs().max() < 1.5e-2 * want.abs().max() and _rel(code.detach(), want.detach()) < 6e-3
    seen = 0
    for name, p in net.named_parameters():
        top, _, rest = name.partition(".")
        if top not in DEPTH_TOPS:
            continue
        if top in TRAINED[guidance]:
            ref = dict(mods[top].named_parameters())[rest].grad
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(ref.norm()) > 0, name
            print(f"{guidance} d {name}: L2 {_rel(p.grad, ref):.3e}")
            assert _rel(p.grad, ref) < 6e-2, (name, _rel(p.grad, ref))
            seen += 1
        else:
            assert p.grad is None, name
    assert seen == (10 if guidance == "sum" else 14)


def test_eval_mode_contract(dev):
    from depthg_amd.featurizer import DinoFeaturizer, DinoFeaturizerWithDepth
    img, depth = inputs(dev)
    plain = build(DinoFeaturizer, tiny_cfg(), dev).eval()
    for guidance in ("sum", "cross_attn"):
        net = build(DinoFeaturizerWithDepth, tiny_cfg(arch="dino_depth", guidance=guidance), dev)
        net.load_state_dict(plain.state_dict(), strict=False)
        assert len(net.train()((img, depth))) == 4
        net.eval()
        with torch.no_grad():
            out = net(img)
            assert len(out) == 3 and out[1].shape == (3, 16, 4, 4)
            if guidance == "sum":                              # the depth is not read: the plain featurizer's code, and no encoder call
                net.depth_downscaling = None
                assert torch.equal(net(img)[1], plain(img)[1]) and torch.equal(out[1], plain(img)[1])
            else:                                              # the learned no-depth row is the query
                image_feat = net._backbone(img)[0]
                want, _ = restate(net, image_feat, None, None, False)
                assert (out[1].cpu() - want).abs().max() < 1.5e-2 * want.abs().max() and _rel(out[1], want) < 6e-3
                net.no_depth_embed.weight.add_(1.0)
                assert not torch.equal(net(img)[1], out[1])


def test_depth_map_of_the_wrong_size_is_refused(dev):
    from depthg_amd.featurizer import DinoFeaturizerWithDepth
    net = build(DinoFeaturizerWithDepth, tiny_cfg(arch="dino_depth", guidance="sum"), dev).train()
    img, _ = inputs(dev)
    with pytest.raises(ValueError, match=r"\(3, 384, 2, 2\).*\(3, 384, 4, 4\)"):
        net((img, torch.rand(3, 1, 16, 16, device=dev)))


def batch(dev, B=4, hw=40, n_classes=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
            "label": torch.randint(0, n_classes, (B, hw, hw), generator=g).to(dev),
            "depth": torch.rand(B, 1, hw, hw, generator=g).to(dev), "depth_pos": torch.rand(B, 1, hw, hw, generator=g).to(dev)}


@pytest.fixture(scope="module")
def default_logs(dev):
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(11)
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(feature_samples=5)).to(dev).train()
    loss, logs = seg.training_step(batch(dev))
    return loss, set(logs)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("guidance", ["none", "concat", "sum", "cross_attn"])
def test_training_step_per_guidance(guidance, fused, dev, default_logs):
    from depthg_amd.segmenter import StandInFeaturizerWithDepth, UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(11)
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", guidance=guidance, dg_fused_adam=fused, feature_samples=5)).to(dev).train()
    assert isinstance(seg.net, StandInFeaturizerWithDepth)
    before = {n: p.detach().clone() for n, p in seg.net.named_parameters()}
    loss, logs = seg.training_step(batch(dev))
    assert bool(torch.isfinite(loss)) and set(logs) == default_logs[1]
    stepped = {id(p) for o in seg.optimizers() for grp in o.param_groups for p in grp["params"]}
    assert [id(p) for p in seg.all_reduced_parameters()] == [id(p) for o in seg.optimizers() for grp in o.param_groups for p in grp["params"]]
    for n, p in seg.net.named_parameters():
        top = n.split(".")[0]
        if top in DEPTH_TOPS:
            trained = top in TRAINED[guidance]
            assert p.requires_grad == trained and (id(p) in stepped) == trained, n
            assert torch.equal(p, before[n]) != trained, (guidance, n)
        elif top in ("cluster1", "cluster2"):
            assert id(p) in stepped and not torch.equal(p, before[n]), n
        else:
            assert torch.equal(p, before[n]), n


def test_default_step_is_unchanged(dev, default_logs):
    print("default step loss", float(default_logs[0]).hex())
    assert float(default_logs[0]).hex() == PINNED_LOSS
