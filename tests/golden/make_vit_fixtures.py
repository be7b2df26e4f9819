"""Golden vectors for depthg_amd/vit.py and featurizer.DinoFeaturizer, captured by IMPORTING the reference on CPU (build container
only): the vendored ViT (src/dino/vision_transformer.py:68-280) and DinoFeaturizer.forward (src/modules.py:90-137).

    tiny_*      a ViT of embed 128, 2 heads, depth 2, patch 8, trained size 32 with seeded weights (attention_reference.seed_module:
                the seed and a checksum are stored, not the 1.7 MB state dict) on a 2 x 3 x 40 x 56 input - not the trained square, so
                the +0.1 bicubic interpolation of the position embeddings runs: feat / attn / qkv of get_intermediate_feat(n=1),
                forward(), the interpolated pos_embed
    keys_*      state_dict names and shapes ("name:d0,d1,...") of vit_small / vit_base at patch 8 / 16
    dino_feat_* DinoFeaturizer eval outputs (cfg.dropout = False) on the tiny backbone, dino_feat_type "feat"
    dino_KK_*   the same for "KK" on a six-head variant (embed 384, depth 1): the reference hard-codes 6 heads there (:113)
DinoFeaturizer cannot be constructed here (its __init__ downloads weights), so, as make_head_fixtures.py does, its `forward` is
called unbound on a stand-in that carries what the method reads.

    python tests/golden/make_vit_fixtures.py     # writes tests/golden/vit.npz
"""
import os
import sys
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as mf  # noqa: E402
import attention_reference as AR  # noqa: E402

VIT_SEED, HEAD_SEED, DIM = 1601, 785, 70


def main():
    M, _ = mf.import_reference()
    import dino.vision_transformer as V
    ln = partial(torch.nn.LayerNorm, eps=1e-6)
    fx = {"vit_seed": np.int64(VIT_SEED), "head_seed": np.int64(HEAD_SEED), "dim": np.int64(DIM)}
    g = torch.Generator().manual_seed(197)
    x = torch.randn(2, 3, 40, 56, generator=g)
    fx["x"] = x.numpy()

    tiny = V.VisionTransformer(qkv_bias=True, norm_layer=ln, mlp_ratio=4, **AR.TINY).eval()
    AR.seed_module(tiny, VIT_SEED)
    fx["tiny_checksum"] = np.asarray(AR.checksum(tiny.state_dict()))
    with torch.no_grad():
        feat, attn, qkv = tiny.get_intermediate_feat(x, n=1)
        fx["tiny_feat"], fx["tiny_attn"], fx["tiny_qkv"] = feat[0].numpy(), attn[0].numpy(), qkv[0].contiguous().numpy()
        fx["tiny_forward"] = tiny(x).numpy()
        fx["tiny_pos_embed"] = tiny.interpolate_pos_encoding(tiny.patch_embed(x).new_zeros(2, 36, 128), 40, 56).numpy()
        fx["tiny_last_attn"] = tiny.get_last_selfattention(x).numpy()

    for arch in ("vit_small", "vit_base"):
        for p in (8, 16):
            sd = V.__dict__[arch](patch_size=p, num_classes=0).state_dict()
            fx[f"keys_{arch}_{p}"] = np.asarray([k + ":" + ",".join(str(d) for d in v.shape) for k, v in sd.items()])

    six = V.VisionTransformer(qkv_bias=True, norm_layer=ln, mlp_ratio=4, **AR.TINY6).eval()
    AR.seed_module(six, VIT_SEED)
    fx["tiny6_checksum"] = np.asarray(AR.checksum(six.state_dict()))
    for feat_type, model in (("feat", tiny), ("KK", six)):
        st = SimpleNamespace(dim=DIM)
        C = model.embed_dim
        head = torch.nn.Module()
        head.cluster1 = M.DinoFeaturizer.make_clusterer(st, C)
        head.cluster2 = M.DinoFeaturizer.make_nonlinear_clusterer(st, C)
        AR.seed_module(head, HEAD_SEED)
        fx[f"dino_{feat_type}_head_checksum"] = np.asarray(AR.checksum(head.state_dict()))
        st.cluster1, st.cluster2, st.model = head.cluster1, head.cluster2, model
        st.patch_size, st.feat_type, st.proj_type = 8, feat_type, "nonlinear"
        st.cfg = SimpleNamespace(model_type="vit_small", dropout=False)
        st.dropout = torch.nn.Dropout2d(p=.1)
        st.dropout.eval()
        st.training = False
        with torch.no_grad():
            feats, code = M.DinoFeaturizer.forward(st, x)
            cls = M.DinoFeaturizer.forward(st, x, return_class_feat=True)
        fx[f"dino_{feat_type}_feats"], fx[f"dino_{feat_type}_code"] = feats.contiguous().numpy(), code.numpy()
        fx[f"dino_{feat_type}_class"] = cls.contiguous().numpy()
        print(feat_type, tuple(feats.shape), tuple(code.shape), tuple(cls.shape))
    out = os.path.join(HERE, "vit.npz")
    np.savez_compressed(out, **fx)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
