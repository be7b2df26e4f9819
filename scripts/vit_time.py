#!/usr/bin/env python3
"""Time the frozen backbone of one training step on the MI355X: the forward of BOTH featurizer passes (img and img_pos,
src/train_segmentation.py:194-212) of vit_small(8) at B = 32, 224 x 224 and 320 x 320, seeded random weights, under no_grad.
One JSON line per form and size, printed and appended to profiles/vit_time.jsonl:

    materialised     the reference's formulation (src/dino/vision_transformer.py:80-92): the (B, heads, N, N) fp32 matrix written
                     and read back - the default path of depthg_amd/vit.py, the baseline
    sdpa_fp32        torch.nn.functional.scaled_dot_product_attention on fp32 q, k, v
    sdpa_bf16        the same on q, k, v cast to bf16 (result cast back to fp32)
    dg_fused         cfg.dg_fused_attention: ops.attention_forward (k_attn_pack + k_attn_fwd)
    dg_fused_linear  cfg.dg_fused_attention + cfg.dg_fused_linear: the blocks' linear layers, LayerNorms, GELU and residual adds
                     through ops.vit_linear_forward (k_lin_fwd) as well
    torch_bf16       torch's own route, for honesty: the whole backbone .to(bfloat16) on a bf16 input with bf16 SDPA (the residual
                     stream, LayerNorm and GELU in bf16 too: less precise than dg_fused_linear, whose stream stays fp32)

All six in one process; host clock around `--steps` double passes ending in a device synchronise, after warm-up of every form and
size; the forms alternate and each is repeated `--repeats` times: median [min, max] in milliseconds.  The line of dg_fused also
carries the algorithmic FLOPs of its attention (4 * B * heads * N^2 * 64 per block) for use with a kernel trace.  Needs the GPU.

    python scripts/vit_time.py [--steps 5] [--repeats 5] [--warmup 2] [--batch 32] [--sizes 224 320] [--out profiles/vit_time.jsonl]
    python scripts/vit_time.py --only dg_fused --sizes 224 --steps 2 --repeats 1      # the run to put under rocprofv3 --kernel-trace --stats
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from depthg_amd import vit  # noqa: E402


def sdpa_attention(dtype):
    def attention(qkv_packed, heads, scale, fused=False):
        B, N, C3 = qkv_packed.shape
        qkv = qkv_packed.reshape(B, N, 3, heads, C3 // (3 * heads)).permute(2, 0, 3, 1, 4)
        q, k, v = (t.to(dtype) for t in (qkv[0], qkv[1], qkv[2]))
        x = F.scaled_dot_product_attention(q, k, v, scale=scale).to(torch.float32)
        return x.transpose(1, 2).reshape(B, N, C3 // 3), None, qkv
    return attention


def clock(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[224, 320])
    ap.add_argument("--only", default=None, help="time this form alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vit_time.py: needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit.vit_small(8).to(dev).eval()
    torch_attention = vit.attention
    model_bf16 = copy.deepcopy(model).to(torch.bfloat16)

    def sdpa_native(qkv_packed, heads, scale, fused=False):
        B, N, C3 = qkv_packed.shape
        qkv = qkv_packed.reshape(B, N, 3, heads, C3 // (3 * heads)).permute(2, 0, 3, 1, 4)
        x = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], scale=scale)
        return x.transpose(1, 2).reshape(B, N, C3 // 3), None, qkv

    def run(form, x, x_pos):
        if form == "torch_bf16":
            vit.attention = sdpa_native
            try:
                with torch.no_grad():
                    return model_bf16.forward_feats(x.to(torch.bfloat16)).float(), model_bf16.forward_feats(x_pos.to(torch.bfloat16)).float()
            finally:
                vit.attention = torch_attention
        model.fused_attention = form in ("dg_fused", "dg_fused_linear")
        model.fused_linear = form == "dg_fused_linear"
        vit.attention = {"sdpa_fp32": sdpa_attention(torch.float32), "sdpa_bf16": sdpa_attention(torch.bfloat16)}.get(form, torch_attention)
        try:
            with torch.no_grad():
                return model.forward_feats(x), model.forward_feats(x_pos)
        finally:
            vit.attention = torch_attention
            model.fused_attention = model.fused_linear = False

    names = ["materialised", "sdpa_fp32", "sdpa_bf16", "dg_fused", "dg_fused_linear", "torch_bf16"]
    if args.only:
        names = [args.only]
    lines = []
    for size in args.sizes:
        g = torch.Generator().manual_seed(size)
        x = torch.randn(args.batch, 3, size, size, generator=g).to(dev)
        x_pos = torch.randn(args.batch, 3, size, size, generator=g).to(dev)
        N = (size // 8) ** 2 + 1
        forms = {k: (lambda k=k: run(k, x, x_pos)) for k in names}
        exact = run("materialised", x, x_pos)[0] if not args.only else None
        for fn in forms.values():
            clock(fn, args.warmup)
        times = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, fn in forms.items():
                times[k].append(clock(fn, args.steps))
        base = statistics.median(times[names[0]])
        for k, ts in times.items():
            line = {"form": k, "model": "vit_small(8), seeded random weights", "batch": args.batch, "size": size, "tokens": N,
                    "what": "forward of both featurizer passes (2 x 12 blocks), no_grad", "steps": args.steps, "repeats": len(ts),
                    "ms_median": round(statistics.median(ts), 2), "ms_min": round(min(ts), 2), "ms_max": round(max(ts), 2),
                    f"vs_{names[0]}": round(statistics.median(ts) / base, 4)}
            if exact is not None:
                got = forms[k]()[0]
                line["rel_l2_vs_materialised"] = float((got - exact).norm() / exact.norm())
            if k == "dg_fused_linear":
                line["linear_gflop_per_double_pass"] = round(2 * 12 * 2 * args.batch * N * 12 * 384 * 384 / 1e9, 1)
            if k == "dg_fused":
                line["attention_gflop_per_double_pass"] = round(2 * 12 * 4 * args.batch * 6 * N * N * 64 / 1e9, 1)
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
