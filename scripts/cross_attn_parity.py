"""Error ratios of the fused cross-attention's arithmetic against the float64 truth, in units of the bf16-operand yardstick, over the
grid of tests/xattn_reference.py -> profiles/cross_attn_parity.md.

    python scripts/cross_attn_parity.py            the CPU emulation (random 0 / 1 masks); needs no GPU
    python scripts/cross_attn_parity.py --gpu      also the kernels (ops.xattn_forward / xattn_backward, the exported mask)
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import xattn_reference as R  # noqa: E402

NAMES = ("o", "dq", "dk", "dv")


def emulation_ratios(case, seed=0):
    q, k, v, g = R.make_inputs(case)
    mask = R.random_mask(case, seed)
    p, heads = case[4], case[3]
    truth, yard = R.attention_f64(q, k, v, g, heads, mask, p), R.attention_f64(q, k, v, g, heads, mask, p, round_bf16=True)
    return R.judge(R.emulate(q, k, v, g, heads, mask, p), truth, yard)


def kernel_ratios(case, seed=1234):
    from depthg_amd import ops
    dev = torch.device("cuda:0")
    q, k, v, g = R.make_inputs(case)
    nq, nk, B, heads, p, _ = case
    mask = ops.xattn_keep_mask(seed, B, heads, nq, nk, p, dev).cpu()
    qd, kd, vd, gd = (t.to(dev) for t in (q, k, v, g))
    o, lse = ops.xattn_forward(qd, kd, vd, heads, p, seed, want_lse=True)
    dq, dk, dv = ops.xattn_backward(qd, kd, vd, o, lse, gd, heads, p, seed)
    truth, yard = R.attention_f64(q, k, v, g, heads, mask, p), R.attention_f64(q, k, v, g, heads, mask, p, round_bf16=True)
    return R.judge(dict(o=o, dq=dq, dk=dk, dv=dv), truth, yard)


def table(fn):
    worst, rows = {n: 0.0 for n in NAMES}, []
    for case in R.GRID:
        j = fn(case)
        rows.append("| " + R.case_id(case) + " | " + " | ".join(f"{j[n][3]:.3f}" for n in NAMES) + " |")
        for n in NAMES:
            worst[n] = max(worst[n], j[n][3])
    return worst, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_attn_parity.md"))
    a = ap.parse_args()
    text = ["# Fused cross-attention: error against float64 in units of the bf16-operand yardstick", "",
            "ratio = (|x - truth| - floor) / |yardstick - truth|, L2 norms over the tensor (tests/xattn_reference.py); a case whose truth",
            "cancels to nothing (one key, one dominant key: dQ and dK) has ratio 0 when the error is under the floor.", "",
            f"Bounds of tests/test_gpu_cross_attn.py: O {R.FACTOR_O}; " +
            ", ".join(f"{n} {R.EMULATED_GRAD[n]} x 1.25 = {R.FACTOR_GRAD[n]:.4f}" for n in ("dq", "dk", "dv")), ""]
    forms = [("CPU emulation of the prescribed arithmetic (random masks)", emulation_ratios)]
    if a.gpu:
        forms.append(("The kernels on an MI355X (exported Philox mask)", kernel_ratios))
    for title, fn in forms:
        worst, rows = table(fn)
        text += [f"## {title}", "", "worst over the grid: " + ", ".join(f"{n} {worst[n]:.3f}" for n in NAMES), "",
                 "| case | O | dQ | dK | dV |", "|---|---|---|---|---|"] + rows + [""]
        print(title, {n: round(worst[n], 4) for n in NAMES})
    with open(a.out, "w") as f:
        f.write("\n".join(text))


if __name__ == "__main__":
    main()
