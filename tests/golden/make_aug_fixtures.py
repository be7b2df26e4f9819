"""Golden vectors of the augmentation-alignment term (src/train_segmentation.py:400-411) by IMPORTING the reference on the CPU (build
container only):

    python tests/golden/make_aug_fixtures.py            # rewrites tests/golden/aug_alignment.npz

Two small cases - a square code map, and a (7, 9) code map next to a 6 x 6 code_aug - with seeded inputs, the coordinates of a
crop-and-flip (depthg_amd.aug_loss.crop_flip_coords), and what the reference's own resize, sample and norm (modules re-exports
utils.resize) give under autograd: the loss and both gradients.  The chain's few calls are the caller's lines; no reference source is
copied.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_fixtures import OUT, import_reference  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from depthg_amd.aug_loss import crop_flip_coords  # noqa: E402

# name: (B, D, (h, w), n, (H, W), boxes, flips)
CASES = {"square": (2, 6, (5, 5), 5, (20, 20), [(1.5, 0.0, 17.0, 18.5), (0.0, 2.0, 19.0, 18.0)], [False, True]),
         "nonsquare": (2, 5, (7, 9), 6, (24, 40), [(2.0, 3.0, 21.0, 36.0), (0.5, 0.0, 22.5, 37.0)], [True, False])}


def main():
    M, _ = import_reference()
    out = {}
    for k, (name, (B, D, (h, w), n, (H, W), boxes, flips)) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(77 + k)
        code = (torch.randn(B, D, h, w, generator=g) + 0.5).requires_grad_(True)
        code_aug = (torch.randn(B, D, n, n, generator=g) + 0.5).requires_grad_(True)
        coord_aug = crop_flip_coords(B, H, W, boxes, flips)
        ds = M.resize(coord_aug.permute(0, 3, 1, 2), n).permute(0, 2, 3, 1)
        loss = -torch.einsum("bkhw,bkhw->bhw", M.norm(M.sample(code, ds)), M.norm(code_aug)).mean()
        loss.backward()
        out.update({f"{name}_code": code.detach().numpy(), f"{name}_code_aug": code_aug.detach().numpy(),
                    f"{name}_coord_aug": coord_aug.numpy(), f"{name}_loss": loss.detach().numpy(),
                    f"{name}_d_code": code.grad.numpy(), f"{name}_d_code_aug": code_aug.grad.numpy()})
    np.savez_compressed(os.path.join(OUT, "aug_alignment.npz"), **out)
    print("wrote aug_alignment.npz", {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
