#!/usr/bin/env python3
"""Measure d loss / d feats of the reconstruction term (k_rec_bwd_code<true>, dg_rec_feats_backward) against the float64 restatement
on the MI355X, case by case, next to the float32 torch chain under autograd (the yardstick), and write the table to
profiles/rec_feats_parity.md.  The cases, inputs and figures are those of tests/test_gpu_rec_feats.py (rec_feats_reference.CASES and
the test module's measure()): relative L2; for `aligned`, whose true gradient vanishes, the absolute L2 error of both routes.

    python scripts/rec_feats_parity.py [--out profiles/rec_feats_parity.md]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rec_feats_reference as F  # noqa: E402
import rec_loss_reference as R  # noqa: E402
import test_gpu_rec_feats as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_feats_parity.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rec_feats_parity.py: needs the GPU (the kernels have no CPU path)")
    dev = torch.device("cuda:0")
    rows = ["# Reconstruction loss, d feats: kernel and float32 torch against the float64 restatement", "",
            f"Measured on an AMD Instinct MI355X (gfx950; the runtime's device string: {torch.cuda.get_device_name(0)!r}) by "
            f"scripts/rec_feats_parity.py; the bound of tests/test_gpu_rec_feats.py is {T.MARGIN:g} x the yardstick's error.  "
            "Relative L2; `aligned` (the true gradient vanishes): absolute L2.", "",
            "| case | kind | B | D | C | map | d_feats err kernel | d_feats err torch | ratio |", "|---|---|---|---|---|---|---|---|---|"]
    worst = (0.0, "")
    for shape, kind in F.CASES:
        B, D, C, (h, w) = R.SHAPES[shape]
        m = T.measure(shape, kind, dev)
        if m["ratio"] > worst[0]:
            worst = (m["ratio"], f"{shape}/{kind}")
        rows.append(f"| {shape} | {kind} | {B} | {D} | {C} | {h}x{w} | {m['kernel']:.2e} | {m['yard']:.2e} | {m['ratio']:.2f} |")
        print(rows[-1], flush=True)
    rows += ["", f"Worst ratio: {worst[0]:.2f} ({worst[1]})."]
    print(rows[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
