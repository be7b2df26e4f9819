#!/usr/bin/env python3
"""Write profiles/head_input_grad_parity.md: the figures of tests/test_gpu_head_input_grad.py - the head's d image_feat kernel
against float64 autograd, next to the operand yardstick (tests/head_input_grad_reference.py) - for every case, as
profiles/head_grad_margin.md holds them for the parameter gradients.  Needs the GPU.

    python scripts/head_input_grad_parity.py [--out profiles/head_input_grad_parity.md]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import head_input_grad_reference as R  # noqa: E402
import head_margin_inputs as H  # noqa: E402
import test_gpu_head_input_grad as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_input_grad_parity.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_input_grad_parity.py: needs the GPU")
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    rows = ["# d image_feat of the projection head against float64 autograd", "",
            "Kernel k_head_dx on an MI355X; yardstick: the float64 restatement with bf16 operands "
            "(tests/head_input_grad_reference.py).  Criterion: ratio <= 2 (L2, row, plane), <= 3 (element); L2 <= 2e-2.", "",
            "| case | plan | figure | kernel | yardstick | ratio |", "|---|---|---|---|---|---|"]
    for case in R.CASES:
        plan = H.check_plan(case)
        inp = R.case_reference(case.id).inp
        second_only = case.id == R.SMALL_PAIR.id
        dx, _ = T.run_case(case, inp, dev, True, (False, True) if second_only else (True, True))
        got, images = (dx[1], slice(case.B, 2 * case.B)) if second_only else (torch.cat(dx), slice(None))
        lines, bad = R.compare(case, got, images)
        route = f"{plan.dh_route}, {'step-major' if plan.step_major else 'row-major'}" if case.proj == "nonlinear" else "linear head"
        for line in lines:
            w = line.split()
            fig, k, y, ratio = w[3].rstrip(":"), w[5], w[7], w[9]
            rows.append(f"| {case.id} | {route} | {fig} | {k} | {y} | {ratio} |")
        print(case.id, "ok" if not bad else bad, flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
