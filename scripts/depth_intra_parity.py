#!/usr/bin/env python3
"""Code-gradient error of DepthContrastiveCorrelationLoss against the float64 restatement of the reference class
(tests/depth_intra_reference.py), next to the error of the two-call route it replaces (two ContrastiveCorrelationLoss calls, added -
the loss is linear in the feature correlation) on the same mask-proof inputs (tests/margin_inputs.py): the figures and their ratios,
as a table for profiles/depth_intra_parity.md.  tests/test_gpu_depth_intra.py sets its bound from the worst ratio.  Needs the GPU.

    python scripts/depth_intra_parity.py [--out profiles/depth_intra_parity.md]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import margin_inputs as MI  # noqa: E402
import test_gpu_depth_intra as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_intra_parity.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_intra_parity.py: needs the GPU (the loss has no CPU path)")
    dev = torch.device("cuda:0")
    rows, worst = [], 0.0
    for case in T.DECOMP:
        new_s, a_s, b_s, errs, totals = T.decomposition_figures(case[0], dev)
        bits = bool(new_s[0] == a_s[0]) and torch.equal(new_s[1:3], b_s[1:3]) and torch.equal(new_s[4:7], b_s[4:7])
        for k, which in enumerate(("code", "code_pos")):
            for fig in MI.FIGURES:
                n, t = getattr(errs["new"][k], fig), getattr(errs["two"][k], fig)
                worst = max(worst, n / t)
                rows.append(f"| {case[0]} | d/d {which} | {fig} | {n:.3e} | {t:.3e} | {n / t:.3f} |")
        rows.append(f"| {case[0]} | total | new {totals[0]:.9e} | two-call {totals[1]:.9e} | float64 {totals[2]:.9e} | loss and cd means bit-equal: {bits} |")
    text = ("# DepthContrastiveCorrelationLoss: code gradients against the float64 restatement\n\n"
            "One call of the new class against the two ContrastiveCorrelationLoss calls it replaces, both against\n"
            "tests/depth_intra_reference.py in float64, on mask-proof inputs (tests/margin_inputs.py); figures of margin_inputs.grad_errors.\n"
            "Written by scripts/depth_intra_parity.py on an MI355X.\n\n"
            "| case | gradient | figure | new class | two-call route | ratio |\n|---|---|---|---|---|---|\n" + "\n".join(rows) +
            f"\n\nWorst ratio: {worst:.3f}.  tests/test_gpu_depth_intra.py holds the new class to GRAD_FACTOR = {T.GRAD_FACTOR} x the two-call route's figure.\n")
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
