#!/usr/bin/env python3
"""Measure the contrastive CRF loss kernels against the float64 restatement on the MI355X, case by case, next to the float32 torch
chain (the yardstick), and write the table to profiles/crf_loss_parity.md.  The cases, inputs and figures are those of
tests/test_gpu_crf_loss.py (its CASES and measure()): loss error = |loss - truth| over the mean |sims K|, d code error = relative L2.

    python scripts/crf_loss_parity.py [--out profiles/crf_loss_parity.md]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_crf_loss as T  # noqa: E402


def ratio(a, b):
    return "inf" if b == 0 and a > 0 else ("1.00" if a == b else f"{a / b:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_loss_parity.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crf_loss_parity.py: needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    rows = ["# Contrastive CRF loss: kernels and float32 torch against the float64 restatement", "",
            f"Measured on an AMD Instinct MI355X (gfx950; the runtime's device string: {torch.cuda.get_device_name(0)!r}) by scripts/crf_loss_parity.py; B = {T.B}; the bound of tests/test_gpu_crf_loss.py "
            f"is {T.MARGIN:g} x the yardstick's error.", "",
            "Where the true d code vanishes (below one float32 spacing of its no-cancellation scale) the relative errors are noise on both sides; "
            f"the last column then gives the kernels' largest |d code| in float32 spacings of that scale (bound {T.NOISE_ULPS:g}).", "",
            "| case | scalars | D | code | image | size | n | loss | loss err kernel | loss err torch | ratio | d code err kernel | d code err torch | ratio | vanishing: spacings |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    worst = {"loss": (0.0, ""), "grad": (0.0, "")}
    for shape, sset in T.CASES:
        D, (h, w), (H, W), size, n, _ = T.SHAPES[shape]
        m = T.measure(shape, sset, dev)
        van = f"{m['grad_kernel_max'] / (T.ULP32 * m['grad_scale']):.3f}" if m["grad_true_max"] < T.ULP32 * m["grad_scale"] else ""
        rl, rg = ratio(m["loss_err_kernel"], m["loss_err_yard"]), ratio(m["grad_err_kernel"], m["grad_err_yard"])
        for key, r in (("loss", rl), ("grad", rg)):
            v = float(r)
            if v > worst[key][0]:
                worst[key] = (v, f"{shape}/{sset}")
        rows.append(f"| {shape} | {sset} | {D} | {h}x{w} | {H}x{W} | {size} | {n} | {m['loss']:.6e} | {m['loss_err_kernel']:.2e} | "
                    f"{m['loss_err_yard']:.2e} | {rl} | {m['grad_err_kernel']:.2e} | {m['grad_err_yard']:.2e} | {rg} | {van} |")
        print(rows[-1], flush=True)
    rows += ["", f"Worst ratios: loss {worst['loss'][0]:.2f} ({worst['loss'][1]}), d code {worst['grad'][0]:.2f} ({worst['grad'][1]})."]
    print(rows[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
