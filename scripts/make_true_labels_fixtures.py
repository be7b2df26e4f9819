"""Generate tests/golden/true_labels_*.npz on the CPU: the reference's ContrastiveCorrelationLoss (src/modules.py:1221-1367) on the
signal cfg.use_true_labels hands it - one_hot_feats(label + 1, n_classes + 1), src/train_segmentation.py:219-225 - at the labels' own
resolution over 8 x 8 code maps.  The reference is imported from a checkout at run time (the import recipe of
tests/golden/make_fixtures.py); only arrays are written: labels, depth, the coordinates and batch maps the reference drew, the eight
loss outputs (means, and every 37th element of the un-reduced tensors), the weighted total and the code gradients.

    python scripts/make_true_labels_fixtures.py [--reference DIR]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

SUB = 37
# name: (label H, W), channels K = n_classes + 1, depth_sampling, depth term, zero_clamp - every factor at both levels on both sizes
CASES = {
    "32x32_k4_fps_depth": ((32, 32), 4, "fps", True, True),
    "32x32_k28_none_depth": ((32, 32), 28, "none", True, True),
    "32x32_k4_none_nodepth_nozc": ((32, 32), 4, "none", False, False),
    "32x32_k28_fps_nodepth": ((32, 32), 28, "fps", False, True),
    "64x72_k4_none_depth_nozc": ((64, 72), 4, "none", True, False),
    "64x72_k28_fps_depth": ((64, 72), 28, "fps", True, True),
    "64x72_k4_fps_nodepth_nozc": ((64, 72), 4, "fps", False, False),
    "64x72_k28_none_nodepth": ((64, 72), 28, "none", False, True),
}
B, D, CODE_HW = 2, 24, (8, 8)


def draw_labels(g, n_classes, H, W):
    """Blocky label maps with values in [-1, n_classes - 1]: 8 x 8 regions, a tenth of the pixels redrawn."""
    coarse = torch.randint(-1, n_classes, (B, (H + 7) // 8, (W + 7) // 8), generator=g)
    label = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]
    noise = torch.randint(-1, n_classes, (B, H, W), generator=g)
    return torch.where(torch.rand(B, H, W, generator=g) < 0.1, noise, label).contiguous()


def run_reference(M, one_hot, cfg, n_classes, label, label_pos, code, code_pos, depth, depth_pos, rng_seed):
    rec = {"rand": [], "perm": [], "fps": []}
    orig_rand, orig_sp, orig_fpsd = torch.rand, M.super_perm, M.farthest_point_sampling_depth

    def rand_wrap(*a, **k):
        rec["rand"].append(orig_rand(*a, **k))
        return rec["rand"][-1]

    def sp_wrap(size, device):
        rec["perm"].append(orig_sp(size, device))
        return rec["perm"][-1]

    def fpsd_wrap(*a, **k):
        rec["fps"].append(orig_fpsd(*a, **k))
        return rec["fps"][-1]

    c, cp = code.clone().requires_grad_(True), code_pos.clone().requires_grad_(True)
    signal, signal_pos = one_hot(label + 1, n_classes + 1), one_hot(label_pos + 1, n_classes + 1)
    torch.manual_seed(rng_seed)
    torch.rand, M.super_perm, M.farthest_point_sampling_depth = rand_wrap, sp_wrap, fpsd_wrap
    try:
        out = M.ContrastiveCorrelationLoss(cfg)(signal, signal_pos, None, None, c, cp, depth, depth_pos)
    finally:
        torch.rand, M.super_perm, M.farthest_point_sampling_depth = orig_rand, orig_sp, orig_fpsd
    src = rec["fps"] if cfg.depth_sampling == "fps" else rec["rand"]
    coords1, coords2 = src[0].clone() * 2 - 1, src[1].clone() * 2 - 1
    # the caller's arithmetic, src/train_segmentation.py:303-350
    total = cfg.pos_inter_weight * out[2].mean() + cfg.pos_intra_weight * out[0].mean() + cfg.neg_inter_weight * out[4].mean()
    if cfg.depth_feat_correlation_loss:
        total = total + cfg.depth_feat_weight * out[6].mean()
    total = total * cfg.correspondence_weight
    total.backward()
    import make_fixtures as MF
    res = {k: np.asarray(getattr(cfg, k)) for k in MF.CFG_KEYS}
    res.update(n_classes=np.asarray(n_classes), label=label.numpy().astype(np.int16), label_pos=label_pos.numpy().astype(np.int16),
               code=code.numpy(), code_pos=code_pos.numpy(), depth=depth.numpy(), depth_pos=depth_pos.numpy(),
               coords1=coords1.numpy(), coords2=coords2.numpy(), perms=torch.stack(rec["perm"]).numpy(),
               pos_intra_loss=out[0].detach().numpy(), pos_inter_loss=out[2].detach().numpy(),
               neg_inter_loss_mean=out[4].mean().detach().numpy(), pos_intra_cd_mean=out[1].mean().detach().numpy(),
               pos_inter_cd_mean=out[3].mean().detach().numpy(), neg_inter_cd_mean=out[5].mean().detach().numpy(),
               total=total.detach().numpy(), grad_code=c.grad.numpy(), grad_code_pos=cp.grad.numpy(),
               store_full=np.asarray(False), sub=np.asarray(SUB))
    names, tens = ["pos_intra_cd", "pos_inter_cd", "neg_inter_loss", "neg_inter_cd"], [out[1], out[3], out[4], out[5]]
    if cfg.depth_feat_correlation_loss:
        res.update(depth_feat_loss=out[6].detach().numpy(), depth_feat_cd_mean=out[7].mean().detach().numpy())
        names.append("depth_feat_cd")
        tens.append(out[7])
    for n, t in zip(names, tens):
        res[n] = t.detach().reshape(-1)[::SUB].numpy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DEPTHG_REFERENCE"), help="the reference checkout (default: make_fixtures.REF)")
    args = ap.parse_args()
    import make_fixtures as MF
    if args.reference:
        MF.REF = args.reference
    M, _ = MF.import_reference()
    import utils as U          # the reference's src/utils.py: one_hot_feats (:64-65)
    torch.set_num_threads(4)
    for i, (name, ((H, W), K, sampling, depth_term, zero_clamp)) in enumerate(CASES.items()):
        n_classes = K - 1
        g = torch.Generator().manual_seed(4100 + i)
        label, label_pos = draw_labels(g, n_classes, H, W), draw_labels(g, n_classes, H, W)
        code, code_pos = torch.randn(B, D, *CODE_HW, generator=g), torch.randn(B, D, *CODE_HW, generator=g)
        # depth at the labels' resolution (the sampler's pooling is then the identity), 8-bit values with a zero block
        depth, depth_pos = (torch.randint(0, 256, (B, 1, H, W), generator=g).float() for _ in range(2))
        depth[:, :, : H // 4, : W // 3] = 0.0
        cfg = MF.make_cfg(depth_sampling=sampling, depth_feat_correlation_loss=depth_term, zero_clamp=zero_clamp, neg_samples=3)
        res = run_reference(M, U.one_hot_feats, cfg, n_classes, label, label_pos, code, code_pos, depth, depth_pos, rng_seed=50 + i)
        path = os.path.join(ROOT, "tests", "golden", f"true_labels_{name}.npz")
        np.savez_compressed(path, **res)
        print(f"{name}: total {float(res['total']):.6f}, |grad_code| {float(np.linalg.norm(res['grad_code'])):.4e}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
