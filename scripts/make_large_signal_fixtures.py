"""Generate tests/golden/large_signal_*.npz on the CPU: the reference's ContrastiveCorrelationLoss on the one-hot label signal of
cfg.use_true_labels at signal sizes above 16384 positions - the sizes the loss's sampler reads in place (k_sample_direct) - over 8 x 8
code maps.  The recipe is scripts/make_true_labels_fixtures.py's (the reference imported from a checkout at run time, arrays only:
labels as int16, the draws, the eight outputs with every 37th element of the un-reduced tensors, the total, the code gradients).

    python scripts/make_large_signal_fixtures.py [--reference DIR]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import make_true_labels_fixtures as TL  # noqa: E402

# name: (label H, W), channels K = n_classes + 1, depth_sampling, depth term, zero_clamp, feature_samples
CASES = {
    "136x124_k28_fps_depth": ((136, 124), 28, "fps", True, True, 11),
    "136x124_k4_none_nodepth_nozc": ((136, 124), 4, "none", False, False, 11),
    "256x256_k28_none_depth": ((256, 256), 28, "none", True, True, 11),
    "136x124_k4_fps_depth_S14": ((136, 124), 4, "fps", True, True, 14),      # above 160 positions: the blob path behind k_gather_norm
}
MAX_BYTES = 1 << 20


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
    B, D, CODE_HW = TL.B, TL.D, TL.CODE_HW
    for i, (name, ((H, W), K, sampling, depth_term, zero_clamp, S)) in enumerate(CASES.items()):
        n_classes = K - 1
        g = torch.Generator().manual_seed(4200 + i)
        label, label_pos = TL.draw_labels(g, n_classes, H, W), TL.draw_labels(g, n_classes, H, W)
        code, code_pos = torch.randn(B, D, *CODE_HW, generator=g), torch.randn(B, D, *CODE_HW, generator=g)
        depth, depth_pos = (torch.randint(0, 256, (B, 1, H, W), generator=g).float() for _ in range(2))
        depth[:, :, : H // 4, : W // 3] = 0.0
        cfg = MF.make_cfg(depth_sampling=sampling, depth_feat_correlation_loss=depth_term, zero_clamp=zero_clamp, neg_samples=3,
                          feature_samples=S)
        res = TL.run_reference(M, U.one_hot_feats, cfg, n_classes, label, label_pos, code, code_pos, depth, depth_pos, rng_seed=70 + i)
        path = os.path.join(ROOT, "tests", "golden", f"large_signal_{name}.npz")
        np.savez_compressed(path, **res)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, f"{path}: {size} bytes"
        print(f"{name}: total {float(res['total']):.6f}, |grad_code| {float(np.linalg.norm(res['grad_code'])):.4e}, {size} bytes")


if __name__ == "__main__":
    main()
