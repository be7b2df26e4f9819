#!/usr/bin/env python3
"""Tabulate the fused attention kernel's error against the float64 attention, next to the yardstick of tests/attention_reference.py
(the same float64 attention on q, k, v rounded to bf16) and to torch's own bf16 scaled_dot_product_attention (ungated), then the
whole-model figures of vit_small(8) with seeded random weights.  Markdown on stdout or into the file named.  Needs the GPU.

    python scripts/vit_parity.py [profiles/vit_parity.md]
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attention_reference as AR  # noqa: E402
from depthg_amd import ops, vit  # noqa: E402


def main():
    if not torch.cuda.is_available():
        sys.exit("vit_parity.py: needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    out = ["# Fused attention parity (k_attn_fwd), measured on an MI355X", "",
           "Relative L2 error against float64 attention; yardstick = float64 attention on bf16-rounded q, k, v; the tests hold",
           f"kernel <= {AR.FACTOR} x yardstick (tests/test_gpu_attention.py).  torch bf16 SDPA is reported, not gated.  scale 1/8.", "",
           "| N | heads | B | sigma | yardstick | k_attn_fwd | ratio | torch bf16 SDPA | ratio |", "|---|---|---|---|---|---|---|---|---|"]
    worst = 0.0
    for N in (1, 2, 63, 64, 65, 197, 785, 1601):
        for heads in (1, 6, 12):
            for B in (1, 3):
                for sigma in (1.0, 3.0):
                    qkv = AR.seeded_qkv(B, N, heads, sigma, seed=1000 * N + 10 * heads + B, device=dev)
                    truth = AR.attention_f64(qkv, heads, 0.125)
                    yard = AR.rel_l2(AR.attention_f64(qkv, heads, 0.125, True), truth)
                    err = AR.rel_l2(ops.attention_forward(qkv, heads, 0.125), truth)
                    q, k, v = (t.to(torch.bfloat16) for t in AR.split_qkv(qkv, heads))
                    sd = F.scaled_dot_product_attention(q, k, v, scale=0.125).float().transpose(1, 2).reshape(B, N, heads * 64)
                    e_sd = AR.rel_l2(sd, truth)
                    worst = max(worst, err / yard)
                    out.append(f"| {N} | {heads} | {B} | {sigma:g} | {yard:.3e} | {err:.3e} | {err / yard:.3f} | {e_sd:.3e} | {e_sd / yard:.3f} |")
    qkv = AR.dominant_qkv(2, 197, 6, 77, seed=5, device=dev)
    truth = AR.attention_f64(qkv, 6, 0.125)
    yard, err = AR.rel_l2(AR.attention_f64(qkv, 6, 0.125, True), truth), AR.rel_l2(ops.attention_forward(qkv, 6, 0.125), truth)
    out += ["", f"Dominant-score rows (q = 40 k_77, N = 197, 6 heads, B = 2): yardstick {yard:.3e}, kernel {err:.3e}, ratio {err / yard:.3f}.",
            f"Largest ratio of the table: {worst:.3f}.", "",
            "## Whole model: vit_small(8), seeded random weights, B = 2, final-norm features against the fp32 torch path", "",
            "| input | bf16-operand model (yardstick) | dg_fused_attention | ratio |", "|---|---|---|---|"]
    model = AR.seed_module(vit.vit_small(8), 42).to(dev).eval()
    for hw in ((224, 224), (224, 320)):
        x = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(7)).to(dev)
        with torch.no_grad():
            model.fused_attention = False
            exact = model.forward_feats(x)
            y = AR.bf16_operand_model(model).forward_feats(x)
            model.fused_attention = True
            f = model.forward_feats(x)
        ey, ef = float((y - exact).norm() / exact.norm()), float((f - exact).norm() / exact.norm())
        out.append(f"| {hw[0]} x {hw[1]} | {ey:.3e} | {ef:.3e} | {ef / ey:.3f} |")
    out += ["", "No pretrained DINO checkpoint was available where this was measured: the error on real DINO weights is unmeasured."]
    text = "\n".join(out) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
