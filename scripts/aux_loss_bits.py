#!/usr/bin/env python3
"""The bits of the three auxiliary loss terms (contrastive CRF, augmentation-alignment, reconstruction): for every case of their GPU
tests' tables (tests/test_gpu_crf_loss.py, tests/aug_alignment_reference.py, tests/rec_loss_reference.py; fixed seeds) the forward and
the backward through depthg_amd.ops, and one line per output tensor:

    term  case  tensor  sha256 of its bytes

The kernels use no atomics, so two builds that compute the same thing print the same listing: run it on both and diff.  `--tree`
names the checkout whose depthg_amd package and built library run (default: this one); the cases always come from this checkout's
tests, so a listing of an older build covers the same cases.  Needs the GPU.

    python scripts/aux_loss_bits.py [--tree PATH] [--out FILE]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from depthg_amd import ops
    import aug_alignment_reference as RA
    import rec_loss_reference as RR
    import test_gpu_crf_loss as TC

    if not torch.cuda.is_available():
        sys.exit("aux_loss_bits.py: needs the GPU (the fused routes have no CPU path)")
    dev = torch.device("cuda:0")
    up = torch.tensor(0.75, device=dev)                   # the upstream gradient: not 1, so that its factor is in the bits
    lines = []

    def emit(term, case, names, tensors):
        torch.cuda.synchronize()
        for name, t in zip(names, tensors):
            digest = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()
            lines.append(f"{term} {case} {name} {digest}")
            print(lines[-1], flush=True)

    for shape, sset in TC.CASES:
        img, code, coords = (t.to(dev) for t in TC.inputs(shape))
        size = TC.SHAPES[shape][3]
        loss, ws = ops.crf_loss_forward(code, img, coords, size, **TC.SETS[sset])
        emit("crf", f"{shape}/{sset}", ("loss", "d_code"), (loss, ops.crf_loss_backward(ws, coords, tuple(code.shape), size, up)))
    for shape, kind in RA.CASES + [RA.WRAPS_CASE]:
        code, code_aug, coord = (t.to(dev) for t in RA.inputs(shape, kind))
        loss, ws = ops.aug_alignment_forward(code, code_aug, coord)
        emit("aug", f"{shape}/{kind}", ("loss", "d_code", "d_code_aug"), (loss,) + tuple(ops.aug_alignment_backward(ws, code, code_aug, up)))
    for shape, kind in RR.CASES:
        operands = tuple(t.to(dev) for t in RR.operands(shape, kind))
        loss, ws = ops.rec_loss_forward(*operands)
        emit("rec", f"{shape}/{kind}", ("loss", "d_code", "d_weight", "d_bias"), (loss,) + tuple(ops.rec_loss_backward(ws, *operands, up)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
