"""Golden vectors of ContrastiveCRFLoss.forward (src/modules.py:1510-1542) by IMPORTING the reference on the CPU (build container only):

    python tests/golden/make_crf_loss_fixtures.py            # rewrites tests/golden/crf_loss.npz

Inputs, the seed and the reference's (B,n,n) output for the default scalars and for a dense set.  The reference draws its sample
coordinates inside forward (two torch.randint calls), so the seed set in front of the call is part of the fixture: a port that draws in
another order cannot reproduce the tensor.  No reference source is copied.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_fixtures import OUT, import_reference  # noqa: E402

SETS = {"default": dict(alpha=.5, beta=.15, gamma=.05, w1=10.0, w2=3.0, shift=0.0),
        "dense": dict(alpha=200.0, beta=.5, gamma=50.0, w1=10.0, w2=3.0, shift=.3)}


def main():
    M, _ = import_reference()
    B, D, h, w, n, seed = 2, 6, 9, 7, 32, 1234
    g = torch.Generator().manual_seed(99)
    guidance = torch.randn(B, 3, h, w, generator=g)
    clusters = torch.nn.functional.normalize(torch.randn(B, D, h, w, generator=g), dim=1, eps=1e-10)
    out = {"guidance": guidance.numpy(), "clusters": clusters.numpy(), "seed": np.int64(seed), "n": np.int64(n)}
    for name, kw in SETS.items():
        fn = M.ContrastiveCRFLoss(n, kw["alpha"], kw["beta"], kw["gamma"], kw["w1"], kw["w2"], kw["shift"])
        torch.manual_seed(seed)
        out[f"{name}_out"] = fn(guidance, clusters).numpy()
        out[f"{name}_scalars"] = np.asarray([kw[k] for k in ("alpha", "beta", "gamma", "w1", "w2", "shift")], np.float64)
    np.savez_compressed(os.path.join(OUT, "crf_loss.npz"), **out)
    print("wrote crf_loss.npz", {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
