#!/usr/bin/env python3
"""Measure the reconstruction-loss kernels against the float64 restatement on the MI355X, case by case, next to the float32 torch
chain (the yardstick), and write the table to profiles/rec_loss_parity.md.  The cases, inputs and figures are those of
tests/test_gpu_rec_loss.py (rec_loss_reference.CASES and the test module's measure()): loss error = |loss - truth| over the mean |s|,
floored at one float32 spacing of the loss; gradient errors = relative L2 (not listed where the true gradient vanishes).

    python scripts/rec_loss_parity.py [--out profiles/rec_loss_parity.md]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rec_loss_reference as R  # noqa: E402
import test_gpu_rec_loss as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_loss_parity.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rec_loss_parity.py: needs the GPU (the kernels have no CPU path)")
    dev = torch.device("cuda:0")
    keys = ("loss",) + T.GRADS
    rows = ["# Reconstruction loss: kernels and float32 torch against the float64 restatement", "",
            f"Measured on an AMD Instinct MI355X (gfx950; the runtime's device string: {torch.cuda.get_device_name(0)!r}) by "
            f"scripts/rec_loss_parity.py; the bound of tests/test_gpu_rec_loss.py is {T.MARGIN:g} x the yardstick's error.", "",
            "| case | kind | B | D | C | map | loss | " + " | ".join(f"{k} err kernel | {k} err torch | ratio" for k in keys) + " |",
            "|---|---|---|---|---|---|---|" + "---|---|---|" * len(keys)]
    worst = {}
    for shape, kind in R.CASES:
        B, D, C, (h, w) = R.SHAPES[shape]
        m = T.measure(shape, kind, dev)
        cells = []
        for key in keys:
            if kind == "aligned" and key != "loss":
                cells.append("- | - | -")
                continue
            k, y = m[key + "_err_kernel"], m[key + "_err_yard"]
            r = k / y
            if r > worst.get(key, (0.0, ""))[0]:
                worst[key] = (r, f"{shape}/{kind}")
            cells.append(f"{k:.2e} | {y:.2e} | {r:.2f}")
        rows.append(f"| {shape} | {kind} | {B} | {D} | {C} | {h}x{w} | {m['loss']:.6e} | " + " | ".join(cells) + " |")
        print(rows[-1], flush=True)
    rows += ["", "Worst ratios: " + ", ".join(f"{key} {r:.2f} ({case})" for key, (r, case) in worst.items()) + "."]
    print(rows[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
