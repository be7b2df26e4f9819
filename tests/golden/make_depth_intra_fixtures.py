"""Golden vectors of DepthContrastiveCorrelationLoss (src/modules.py:1370-1463) by IMPORTING the reference class on the CPU (build
container only):

    python tests/golden/make_depth_intra_fixtures.py            # rewrites tests/golden/depth_intra.npz

Three small cases - the default recipe, no-pointwise + no-zero-clamp, stabalize.  The class draws its coordinates and batch maps
itself, so each case seeds torch's generator, replays the class's draws in its order (two torch.rand, then one randperm per negative
with super_perm's bump, :1184-1188, 1424-1425, 1448) to record them, seeds again and calls the class; recorded: the inputs, the draws,
the 6-tuple and the autograd gradients of the caller's weighted total (src/train_segmentation.py:347-350).  No reference source is copied.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_fixtures import OUT, import_reference, make_cfg  # noqa: E402

# name: (B, C, D, hw, S, n_neg, cfg overrides)
CASES = {"default": (2, 16, 6, 7, 5, 2, {}),
         "nopointwise_noclamp": (3, 12, 5, 6, 4, 1, dict(pointwise=False, zero_clamp=False)),
         "stabalize": (2, 16, 6, 7, 5, 2, dict(stabalize=True))}


def main():
    M, _ = import_reference()
    out = {"cases": np.array(list(CASES))}
    for k, (name, (B, C, D, hw, S, N, over)) in enumerate(CASES.items()):
        cfg = make_cfg(feature_samples=S, neg_samples=N, depth_feat_correlation_loss=False, pos_intra_shift=0.18,
                       pos_inter_shift=0.12, neg_inter_shift=0.46, **over)
        g = torch.Generator().manual_seed(4100 + k)
        f, fp, aug, augp = (torch.randn(B, C, hw, hw, generator=g) for _ in range(4))
        aug = 0.6 * f + 0.8 * aug               # (depth-augmented features are the backbone's plus something)
        c = torch.randn(B, D, hw, hw, generator=g).requires_grad_(True)
        cp = torch.randn(B, D, hw, hw, generator=g).requires_grad_(True)
        torch.manual_seed(5200 + k)
        c1 = torch.rand([B, S, S, 2]) * 2 - 1
        c2 = torch.rand([B, S, S, 2]) * 2 - 1
        perms = []
        for _ in range(N):
            perm = torch.randperm(B, dtype=torch.long)
            perm[perm == torch.arange(B)] += 1
            perms.append(perm % B)
        torch.manual_seed(5200 + k)
        res = M.DepthContrastiveCorrelationLoss(cfg)(f, fp, None, None, c, cp, aug, augp)
        total = (cfg.pos_inter_weight * res[2].mean() + cfg.pos_intra_weight * res[0].mean() +
                 cfg.neg_inter_weight * res[4].mean()) * cfg.correspondence_weight
        total.backward()
        p = name + "_"
        out.update({p + "feats": f.numpy(), p + "feats_pos": fp.numpy(), p + "aug": aug.numpy(), p + "aug_pos": augp.numpy(),
                    p + "code": c.detach().numpy(), p + "code_pos": cp.detach().numpy(), p + "coords1": c1.numpy(),
                    p + "coords2": c2.numpy(), p + "perms": torch.stack(perms).numpy(),
                    p + "cfg_flags": np.array([cfg.pointwise, cfg.zero_clamp, cfg.stabalize]),
                    p + "cfg_shifts": np.array([cfg.pos_intra_shift, cfg.pos_inter_shift, cfg.neg_inter_shift]),
                    p + "cfg_weights": np.array([cfg.pos_intra_weight, cfg.pos_inter_weight, cfg.neg_inter_weight, cfg.correspondence_weight]),
                    p + "dims": np.array([S, N]),
                    p + "pos_intra_loss": res[0].detach().numpy(), p + "pos_intra_cd": res[1].detach().numpy(),
                    p + "pos_inter_loss": res[2].detach().numpy(), p + "pos_inter_cd": res[3].detach().numpy(),
                    p + "neg_inter_loss": res[4].detach().numpy(), p + "neg_inter_cd": res[5].detach().numpy(),
                    p + "total": total.detach().numpy(), p + "grad_code": c.grad.numpy(), p + "grad_code_pos": cp.grad.numpy()})
    np.savez_compressed(os.path.join(OUT, "depth_intra.npz"), **out)
    print("wrote depth_intra.npz", os.path.getsize(os.path.join(OUT, "depth_intra.npz")), "bytes")


if __name__ == "__main__":
    main()
