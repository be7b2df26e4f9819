"""A/B fingerprint of the Python binding layer: runs the head, both featurizers and every route of the correlation loss on seeded
inputs and writes the sha256 of every output and gradient tensor, and of torch's generator states behind each case, as JSON.
Only public names are used, so the script runs unchanged on two commits; the two files must be identical when a change to the
binding is meant to leave values, gradients and random draws alone.

    python scripts/binding_ab.py OUT.json
"""
import hashlib
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from depthg_amd import ContrastiveCorrelationLoss, DinoFeaturizer, ops  # noqa: E402
from depthg_amd.head import ProjectionHead, draw_keep_masks, draw_keep_masks_pair  # noqa: E402
from depthg_amd.segmenter import StandInFeaturizer, default_segmenter_cfg  # noqa: E402

DEV = torch.device("cuda:0")
TINY_VIT = dict(img_size=[32], patch_size=8, embed_dim=128, depth=2, num_heads=2)


def sha(t):
    if t is None:
        return None
    if isinstance(t, ops.DeferredDropout):
        return {"feats": sha(t.feats), "keep": sha(t.keep), "scale": t.scale, "materialized": sha(t.materialize())}
    t = t.detach().contiguous().cpu()
    return f"{t.dtype}{tuple(t.shape)}:" + hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def rng_states():
    return {"cuda": sha(torch.cuda.get_rng_state(DEV)), "cpu": sha(torch.get_rng_state())}


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def grads(module):
    return {n: sha(p.grad) for n, p in module.named_parameters() if p.requires_grad}


def backward_through(codes, seed):
    """A fixed random upstream for every code map."""
    sum((c * randn(*c.shape, seed=seed + i)).sum() for i, c in enumerate(codes)).backward()


def head_cases():
    B, C, D, hw = 4, 64, 24, 14
    f, fp = randn(B, C, hw, hw, seed=1), randn(B, C, hw, hw, seed=2)
    out = {}
    for proj in (None, "linear", "nonlinear"):
        for train in (True, False):
            for given in (True, False):
                torch.manual_seed(7)
                head = ProjectionHead(C, D, proj).to(DEV).train(train)
                keeps = draw_keep_masks(B, C, DEV) if given else None
                code, feats = head(f, True, keeps)
                if proj is not None and train:
                    backward_through([code], 20)
                out[f"single/{proj}/train={train}/keeps_given={given}"] = {
                    "code": sha(code), "feats": sha(feats), "grads": grads(head), "rng": rng_states()}
    for proj in ("linear", "nonlinear"):
        for defer in (False, True):
            for given in (True, False):
                torch.manual_seed(8)
                head = ProjectionHead(C, D, proj).to(DEV).train()
                keeps = draw_keep_masks_pair(B, C, DEV) if given else None
                (code, feats), (code_pos, feats_pos) = head.forward_pair(f, fp, True, keeps, defer)
                backward_through([code, code_pos], 30)
                out[f"pair/{proj}/defer={defer}/keeps_given={given}"] = {
                    "code": sha(code), "code_pos": sha(code_pos), "feats": sha(feats), "feats_pos": sha(feats_pos),
                    "grads": grads(head), "rng": rng_states()}
    return out


def featurizer_cases():
    out = {}
    img, img_pos = randn(2, 3, 40, 40, seed=3), randn(2, 3, 40, 40, seed=4)
    for kind in ("standin", "dino"):
        for proj in ("linear", "nonlinear"):
            for train in (True, False):
                torch.manual_seed(9)
                cfg = default_segmenter_cfg(model_type="vit_small", dino_patch_size=8, projection_type=proj,
                                            dg_dino_vit_kwargs=dict(TINY_VIT) if kind == "dino" else None)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    net = (DinoFeaturizer(70, cfg) if kind == "dino" else StandInFeaturizer(70, cfg)).to(DEV).train(train)
                case = {"state_dict_keys": list(net.state_dict().keys()), "parameter_names": [n for n, _ in net.named_parameters()]}
                res = net(img)
                backward_codes = [res[1]]
                case["forward"] = [sha(t) for t in res]
                case["class_feat"] = sha(net(img, return_class_feat=True))
                for defer in (False, True):
                    pair = net.forward_pair(img, img_pos, defer)
                    case[f"forward_pair/defer={defer}"] = [[sha(t) for t in one] for one in pair]
                    backward_codes += [pair[0][1], pair[1][1]]
                if train:
                    backward_through(backward_codes, 40)
                case["grads"], case["rng"] = grads(net), rng_states()
                out[f"{kind}/{proj}/train={train}"] = case
    return out


def loss_cases():
    routes = {
        "small_sample_grid": dict(C=64, hw=14, cfg=dict(feature_samples=11)),
        "dense_identity_draw": dict(C=64, hw=14, cfg=dict(feature_samples=14, dg_dense_grid=True)),
        "dense_identity_draw_graph_safe": dict(C=64, hw=14, cfg=dict(feature_samples=14, dg_dense_grid=True, dg_graph_safe=True)),
        "deferred_dropout_identity": dict(C=64, hw=14, cfg=dict(feature_samples=14, dg_dense_grid=True), defer=True),
        "wide_identity_C1024": dict(C=1024, hw=14, cfg=dict(feature_samples=14, dg_dense_grid=True)),
        "wide_sampled_C1024_20x20_S16": dict(C=1024, hw=20, cfg=dict(feature_samples=16)),
    }
    B, D = 4, 24
    out = {}
    for name, r in routes.items():
        for mode in ("full", "reduced"):
            torch.manual_seed(11)
            C, hw = r["C"], r["hw"]
            f, fp = randn(B, C, hw, hw, seed=5), randn(B, C, hw, hw, seed=6)
            c, cp = randn(B, D, hw, hw, seed=7).requires_grad_(True), randn(B, D, hw, hw, seed=8).requires_grad_(True)
            d = torch.randint(0, 256, (B, 1, 8 * hw, 8 * hw), generator=torch.Generator().manual_seed(9)).float().to(DEV)
            if r.get("defer"):
                ka, kb = draw_keep_masks(B, C, DEV, use=(True, True, False))[:2]
                f, fp = ops.DeferredDropout(f, ka, 1.0 / 0.9), ops.DeferredDropout(fp, kb, 1.0 / 0.9)
            cfg = default_segmenter_cfg(depth_sampling="none", dg_outputs=mode, **r["cfg"])
            loss_fn = ContrastiveCorrelationLoss(cfg)
            res = loss_fn(f, fp, None, None, c, cp, d, d)
            loss_fn.total.backward()
            out[f"{name}/{mode}"] = {"outputs": [sha(t) for t in res], "scalars": sha(loss_fn.scalars), "total": sha(loss_fn.total),
                                     "perms": sha(loss_fn.last_call[1]), "grad_code": sha(c.grad), "grad_code_pos": sha(cp.grad),
                                     "rng": rng_states()}
    return out


def main():
    result = {"head": head_cases(), "featurizers": featurizer_cases(), "loss": loss_cases()}
    torch.cuda.synchronize()
    with open(sys.argv[1], "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(f"binding_ab: {sum(len(v) for v in result.values())} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
