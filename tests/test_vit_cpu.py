"""CPU tests of depthg_amd/vit.py (the DINO ViT, src/dino/vision_transformer.py:68-280) and featurizer.DinoFeaturizer
(src/modules.py:19-137) against vectors from the imported reference (tests/golden/vit.npz, tests/golden/make_vit_fixtures.py).

Both sides of the ViT comparison are the same fp32 torch operations: rtol 1e-5 / atol 1e-6, the scale of this project's CPU
oracle-versus-golden checks.  The head (run_head) has no CPU route, so the featurizer's `code` is compared on the GPU
(tests/test_gpu_attention.py); here the featurizer runs with projection_type None wherever it must produce outputs."""
import urllib.request
import warnings

import numpy as np
import pytest
import torch

import attention_reference as AR
from conftest import load_golden


def _close(got, want):
    return np.allclose(got.detach().numpy(), want, rtol=1e-5, atol=1e-6)


@pytest.fixture(scope="module")
def fx():
    return load_golden("vit.npz")


@pytest.fixture(scope="module")
def tiny(fx):
    from depthg_amd import vit
    return AR.seed_module(vit.VisionTransformer(**AR.TINY), int(fx["vit_seed"]), fx["tiny_checksum"]).eval()


def test_vit_reproduces_reference_vectors(fx, tiny):
    x = torch.from_numpy(fx["x"])
    with torch.no_grad():
        feat, attn, qkv = tiny.get_intermediate_feat(x, n=1)
        assert len(feat) == len(attn) == len(qkv) == 1
        assert tuple(qkv[0].shape) == (3, 2, 2, 36, 64)
        assert _close(feat[0], fx["tiny_feat"]) and _close(attn[0], fx["tiny_attn"]) and _close(qkv[0], fx["tiny_qkv"])
        assert _close(tiny(x), fx["tiny_forward"])
        assert _close(tiny.forward_feats(x), fx["tiny_feat"])
        assert _close(tiny.get_last_selfattention(x), fx["tiny_last_attn"])
        assert _close(tiny.get_intermediate_layers(x, n=1)[0], fx["tiny_feat"])
        two = tiny.get_intermediate_feat(x, n=2)
        assert [len(t) for t in two] == [2, 2, 2] and _close(two[0][1], fx["tiny_feat"])
        pos = tiny.interpolate_pos_encoding(torch.zeros(2, 36, 128), 40, 56)
        assert _close(pos, fx["tiny_pos_embed"])
        # the trained square takes the stored embedding as it is (:182-183)
        assert tiny.interpolate_pos_encoding(torch.zeros(1, 17, 128), 32, 32) is tiny.pos_embed


@pytest.mark.parametrize("arch,patch", [("vit_small", 8), ("vit_small", 16), ("vit_base", 8), ("vit_base", 16)])
def test_state_dict_is_a_dino_checkpoints(fx, arch, patch):
    from depthg_amd import vit
    sd = vit.ARCHS[arch](patch_size=patch).state_dict()
    mine = [k + ":" + ",".join(str(d) for d in v.shape) for k, v in sd.items()]
    assert mine == [str(s) for s in fx[f"keys_{arch}_{patch}"]]


def test_vit_tiny_factory_and_fused_flag_need_head_dim_64():
    from depthg_amd import vit
    m = vit.vit_tiny(16, depth=1)
    assert m.embed_dim == 192 and m.num_heads == 3
    with pytest.raises(ValueError, match="head dimension 64"):
        vit.VisionTransformer(**{**AR.TINY, "num_heads": 4}, fused_attention=True)


def _cfg(**over):
    from depthg_amd.segmenter import default_segmenter_cfg
    return default_segmenter_cfg(**{**dict(model_type="vit_small", dino_patch_size=8, dropout=False, dg_dino_vit_kwargs=dict(AR.TINY)), **over})


def _featurizer(cfg, dim=70):
    from depthg_amd import DinoFeaturizer
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DinoFeaturizer(dim, cfg)


def test_checkpoint_file_loads_and_changes_the_features(fx, tiny, tmp_path):
    x = torch.from_numpy(fx["x"])
    path = tmp_path / "dino.pth"
    torch.save({"teacher": {"module.backbone." + k: v for k, v in tiny.state_dict().items()}}, path)
    plain = tmp_path / "plain.pth"
    torch.save(tiny.state_dict(), plain)
    random_feats = _featurizer(_cfg(projection_type=None)).eval()(x)[0]
    for p in (path, plain):
        with warnings.catch_warnings():
            warnings.simplefilter("error")                 # a given checkpoint: no warning
            from depthg_amd import DinoFeaturizer
            net = DinoFeaturizer(70, _cfg(projection_type=None, pretrained_weights=str(p))).eval()
        feats, code = net(x)
        want = torch.from_numpy(fx["tiny_feat"])[:, 1:, :].reshape(2, 5, 7, -1).permute(0, 3, 1, 2)
        assert _close(feats, want.numpy()) and code is feats
        assert not torch.allclose(feats, random_feats, atol=1e-2)


def test_no_weights_warns_and_opens_no_connection(monkeypatch):
    from depthg_amd import DinoFeaturizer

    def refuse(*a, **k):
        raise AssertionError("a network call was attempted")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", refuse)
    monkeypatch.setattr(urllib.request, "urlopen", refuse)
    with pytest.warns(UserWarning, match="dino_deitsmall8_300ep_pretrain.pth"):
        net = DinoFeaturizer(70, _cfg())
    assert net.n_feats == 128
    with pytest.warns(UserWarning, match="dino_vitbase16_pretrain.pth"):
        DinoFeaturizer(70, _cfg(model_type="vit_base", dino_patch_size=16, dg_dino_vit_kwargs=dict(depth=1)))


def test_dino_featurizer_contract(fx):
    x = torch.from_numpy(fx["x"])
    net = _featurizer(_cfg(projection_type=None))
    net.eval()
    assert len(net(x)) == 2
    net.train()
    out = net(x)
    assert len(out) == 3 and out[2].numel() == 1            # nothing reads the attention: the placeholder
    assert not net.model.training                           # the backbone stays in eval mode (:91)
    pair = net.forward_pair(x, x)
    assert len(pair) == 2 and len(pair[0]) == 3 and net.supports_deferred_dropout
    cls = net(x, return_class_feat=True)
    assert tuple(cls.shape) == (2, 128, 1, 1)
    # lhp with the attention strategy reads it: the last block's probabilities
    lhp = _featurizer(_cfg(projection_type=None, lhp=True, propagation_strategy="attn")).train()
    attn = lhp(x)[2]
    assert tuple(attn.shape) == (2, 2, 36, 36) and torch.allclose(attn.sum(-1), torch.ones(2, 2, 36), atol=1e-5)
    assert lhp.eval()(x)[0].shape == (2, 128, 5, 7)
    # "KK": the last block's keys, heads side by side
    kk = _featurizer(_cfg(projection_type=None, dino_feat_type="KK")).eval()
    assert tuple(kk(x)[0].shape) == (2, 128, 5, 7)
    with pytest.raises(ValueError, match="Unknown feat type"):
        _featurizer(_cfg(projection_type=None, dino_feat_type="QQ")).eval()(x)
    with pytest.raises(ValueError, match="Unknown arch"):
        _featurizer(_cfg(model_type="resnet50"))
    with pytest.raises(AssertionError):
        net(torch.zeros(1, 3, 36, 40))                      # not a multiple of the patch size (:93-94)


def test_kk_matches_reference_features_on_six_heads(fx):
    from depthg_amd import DinoFeaturizer
    with pytest.warns(UserWarning):
        net = DinoFeaturizer(70, _cfg(projection_type=None, dino_feat_type="KK", dg_dino_vit_kwargs=dict(AR.TINY6))).eval()
    AR.seed_module(net.model, int(fx["vit_seed"]), fx["tiny6_checksum"])
    feats, _ = net(torch.from_numpy(fx["x"]))
    assert _close(feats, fx["dino_KK_feats"])
    assert _close(net(torch.from_numpy(fx["x"]), return_class_feat=True), fx["dino_KK_class"])


def test_trainable_parameters_are_the_heads():
    net = _featurizer(_cfg())
    trainable = [n for n, p in net.named_parameters() if p.requires_grad]
    assert trainable == [n for n, _ in net.named_parameters() if n.startswith(("cluster1.", "cluster2."))]
    assert trainable == ["cluster1.0.weight", "cluster1.0.bias", "cluster2.0.weight", "cluster2.0.bias", "cluster2.2.weight", "cluster2.2.bias"]
    assert not any(p.requires_grad for p in net.model.parameters())


def test_segmenter_builds_the_backbone_only_on_request():
    from depthg_amd import DinoFeaturizer
    from depthg_amd.segmenter import StandInFeaturizer, UnsupervisedSegmenter, default_segmenter_cfg
    cfg = default_segmenter_cfg()
    assert cfg.dg_dino_backbone is False and cfg.dg_fused_attention is False
    assert type(UnsupervisedSegmenter(5, cfg).net) is StandInFeaturizer
    with pytest.warns(UserWarning, match="pretrained_weights"):
        seg = UnsupervisedSegmenter(5, _cfg(dg_dino_backbone=True, dg_fused_attention=True))
    assert type(seg.net) is DinoFeaturizer and seg.net.model.fused_attention is True
    assert [tuple(p.shape) for p in seg.head_parameters()] == [(70, 128, 1, 1), (70,), (128, 128, 1, 1), (128,), (70, 128, 1, 1), (70,)]


def test_attention_forward_refuses_before_the_gpu_path():
    from depthg_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attention_forward(torch.zeros(2, 10, 3 * 6 * 64), 6)
    with pytest.raises(ValueError, match="float32"):
        ops.attention_forward(torch.zeros(2, 10, 3 * 6 * 64, dtype=torch.float64), 6)
    with pytest.raises(ValueError, match="head dimension 64"):
        ops.attention_forward(torch.zeros(2, 10, 3 * 6 * 32), 6)
    with pytest.raises(ValueError, match="contiguous"):
        ops.attention_forward(torch.zeros(10, 2, 3 * 6 * 64).transpose(0, 1), 6)
    # the ViT's fused route is the same entry point: no quiet fall-back to torch on the CPU
    from depthg_amd import vit
    with pytest.raises(RuntimeError, match="GPU"):
        vit.VisionTransformer(**AR.TINY, fused_attention=True).eval().forward_feats(torch.zeros(1, 3, 32, 32))


def test_library_declares_the_attention_entry_points():
    from depthg_amd import _lib
    lib = _lib.load()
    assert {"dg_attention_forward", "dg_attention_workspace_bytes"} <= set(_lib.EXPORTS)
    assert lib.dg_attention_workspace_bytes(2, 6, 785) == 2 * 6 * 25 * 8192
    assert lib.dg_attention_workspace_bytes(0, 6, 785) == 0 and lib.dg_attention_workspace_bytes(20000, 6, 10) == 0
    # head dimension 32 is refused before any launch (no GPU is needed to be told so)
    rc = lib.dg_attention_forward(None, 1, 10, 6, 32, 0.125, None, None, 0, None)
    assert rc == -2 and b"head_dim=32" in lib.dg_last_error()
