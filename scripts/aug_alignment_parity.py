#!/usr/bin/env python3
"""Measure the augmentation-alignment kernels against the float64 restatement on the MI355X, case by case, next to the float32 torch
chain (the yardstick), and write the table to profiles/aug_alignment_parity.md.  The cases, inputs and figures are those of
tests/test_gpu_aug_alignment.py (aug_alignment_reference.CASES and the test module's measure()): loss error = |loss - truth| over the
mean |s|, floored at one float32 spacing of the loss; gradient errors = relative L2.

    python scripts/aug_alignment_parity.py [--out profiles/aug_alignment_parity.md]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aug_alignment_reference as R  # noqa: E402
import test_gpu_aug_alignment as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_alignment_parity.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aug_alignment_parity.py: needs the GPU (the kernels have no CPU path)")
    dev = torch.device("cuda:0")
    rows = ["# Augmentation-alignment loss: kernels and float32 torch against the float64 restatement", "",
            f"Measured on an AMD Instinct MI355X (gfx950; the runtime's device string: {torch.cuda.get_device_name(0)!r}) by "
            f"scripts/aug_alignment_parity.py; B = {R.B}; the bound of tests/test_gpu_aug_alignment.py is {T.MARGIN:g} x the yardstick's error.", "",
            "| case | coordinates | D | code | code_aug | coord_aug | loss | loss err kernel | loss err torch | ratio | d code err kernel | d code err torch "
            "| ratio | d code_aug err kernel | d code_aug err torch | ratio |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    worst = {}
    for shape, kind in R.CASES:
        D, (h, w), n, (H, W) = R.SHAPES[shape]
        m = T.measure(shape, kind, dev)
        cells = []
        for key in ("loss", "d_code", "d_code_aug"):
            k, y = m[key + "_err_kernel"], m[key + "_err_yard"]
            r = k / y
            if r > worst.get(key, (0.0, ""))[0]:
                worst[key] = (r, f"{shape}/{kind}")
            cells.append(f"{k:.2e} | {y:.2e} | {r:.2f}")
        rows.append(f"| {shape} | {kind} | {D} | {h}x{w} | {n}x{n} | {H}x{W} | {m['loss']:.6e} | " + " | ".join(cells) + " |")
        print(rows[-1], flush=True)
    rows += ["", "Worst ratios: " + ", ".join(f"{key} {r:.2f} ({case})" for key, (r, case) in worst.items()) + "."]
    print(rows[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
