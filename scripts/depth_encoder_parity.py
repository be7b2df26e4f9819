"""Records the fused depth encoder's parity on the GPU: for the cases of tests/test_gpu_depth_encoder.py, the error of the result and
of the ten gradients against the float64 truth, beside the bf16 yardstick's (tests/depth_encoder_reference.py), as ratios.

    python scripts/depth_encoder_parity.py [--out profiles/depth_encoder_parity.md]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "depth_encoder_parity.md"))
    a = ap.parse_args()
    from depthg_amd import depth_encoder
    from tests import depth_encoder_reference as R
    from tests.test_gpu_depth_encoder import CASES, _inputs
    dev = torch.device("cuda:0")
    lines = ["# Fused depth encoder: parity against the float64 truth", "",
             "Kernel error and bf16-yardstick error (tests/depth_encoder_reference.py), both against float64 autograd of the stack; the",
             f"criterion is kernel <= {R.FACTOR} x yardstick per tensor, in L2 and in the largest element.  L2 figures are relative to the",
             "truth's norm, the largest-element figures absolute.", "",
             "| case (B, h x w, C) | tensor | L2 kernel | L2 yardstick | ratio | max kernel | max yardstick | ratio |", "|---|---|---|---|---|---|---|---|"]
    worst = 0.0
    for B, h, w, C in CASES:
        depth, gout = _inputs(B, h, w, C, 10 + C + B)
        stack = R.make_stack(C, 20 + B)
        out_t, grads_t = R.truth(stack, depth, gout)
        out_y, grads_y = R.yardstick(R.stack_params(stack), depth, gout)
        s = stack.to(dev)
        out = depth_encoder(depth.to(dev), s)
        out.backward(gout.to(dev))
        got = [out.detach()] + [p.grad for p in R.stack_params(s)]
        for name, g, t, y in zip(("out",) + tuple("d " + n for n in R.NAMES), got, [out_t] + grads_t, [out_y] + grads_y):
            kl2, yl2, kmax, ymax = R.errors(g, t, y)
            n = float(t.norm()) or 1.0
            r2, rm = (kl2 / yl2 if yl2 else 0.0), (kmax / ymax if ymax else 0.0)
            worst = max(worst, r2, rm)
            lines.append(f"| ({B}, {h} x {w}, {C}) | {name} | {kl2 / n:.3e} | {yl2 / n:.3e} | {r2:.3f} | {kmax:.3e} | {ymax:.3e} | {rm:.3f} |")
    lines += ["", f"Largest ratio: {worst:.3f}.  No tensor needs more than {R.FACTOR} x."]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
