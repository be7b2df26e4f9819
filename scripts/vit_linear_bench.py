#!/usr/bin/env python3
"""Time the four launches of one fused ViT block's linear layers (ops.vit_linear_forward, k_lin_fwd) one by one on the MI355X, at the
token counts of vit_small(8) with B = 32: N = 785 (224 x 224) and N = 1601 (320 x 320).  Per kind: HIP-event time per launch over
`--launches` back-to-back launches (median of `--repeats`), the algorithmic TFLOP/s against the 2.5 PFLOP/s dense bf16 peak, and the
compulsory bytes (x read once, y written once, the residual read, the packed weight once) per second against the 6.29 TB/s measured
copy rate.  Seeded random operands.  Markdown on stdout or into the file named.  Needs the GPU.

    python scripts/vit_linear_bench.py [out.md] [--launches 20] [--repeats 5]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import linear_reference as LR  # noqa: E402
from depthg_amd import ops  # noqa: E402

LAYERS = [("norm1 + qkv", "ln", 384, 1152), ("proj + residual", "res", 384, 384), ("norm2 + fc1 + GELU -> bf16", "ln_gelu_bf16", 384, 1536),
          ("fc2 (bf16 in) + residual", "bf16_res", 1536, 384)]
PEAK_TFLOPS, COPY_TBS = 2500.0, 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vit_linear_bench.py: needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    out = ["| tokens | layer | K | Nout | us / launch [min, max] | TFLOP/s | of bf16 peak | TB/s | of copy rate | nearer bound |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for N in (785, 1601):
        M = 32 * N
        for name, kind, K, Nout in LAYERS:
            ln, gelu, res, in_bf16, out_bf16 = LR.KINDS[kind]
            c = {k: (v.to(dev) if v is not None else None) for k, v in LR.make_case(kind, M, K, Nout, 1.0, seed=N + K).items()}
            packed = ops.vit_linear_pack(c["w"])
            y = torch.empty(M, Nout, device=dev, dtype=torch.bfloat16 if out_bf16 else torch.float32)
            kw = dict(ln_weight=c["gamma"], ln_bias=c["beta"], gelu=gelu, residual=c["residual"], out=y, out_bf16=out_bf16)
            call = lambda: ops.vit_linear_forward(c["x"], packed, Nout, c["b"], **kw)
            for _ in range(3):
                call()
            ts = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    call()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) / args.launches * 1e3)
            us = statistics.median(ts)
            tf = 2.0 * M * K * Nout / us / 1e6
            nbytes = M * K * (2 if in_bf16 else 4) + M * Nout * (2 if out_bf16 else 4) * (2 if res else 1) + 2 * K * Nout
            tb = nbytes / us / 1e6
            bound = "MFMA" if tf / PEAK_TFLOPS > tb / COPY_TBS else "HBM"
            out.append(f"| {M} | {name} | {K} | {Nout} | {us:.1f} [{min(ts):.1f}, {max(ts):.1f}] | {tf:.0f} | {100 * tf / PEAK_TFLOPS:.1f} % | "
                       f"{tb:.2f} | {100 * tb / COPY_TBS:.1f} % | {bound} |")
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
