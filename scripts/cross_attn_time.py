"""Times the "cross_attn" guidance's attention of a dino_depth step on the GPU: (a) the torch route (nn.MultiheadAttention under
autograd: what cfg.dg_fused_cross_attn = False runs) against (b) the fused HIP route (depthg_amd.multihead_cross_attention), forward
plus backward of one `_cross_attend` at the training shape (B = 32, C = 384, feature grid 28 x 28: 784 queries on 784 keys, 8 heads of
48, training mode, p = 0.1), and a whole `training_step` under guidance "cross_attn" with and without the flag.  Host clock around
CALLS calls between two synchronisations, REPEATS repeats, the forms alternated inside every repeat; median [min, max] per call.
One JSON line per form -> profiles/cross_attn_time.jsonl.

    python scripts/cross_attn_time.py [--out profiles/cross_attn_time.jsonl] [--calls 20] [--repeats 5] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def alternate(forms, calls, repeats, warmup=3):
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            times[k].append(timed(fn, calls))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "cross_attn_time.jsonl"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    from depthg_amd import multihead_cross_attention
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    dev = torch.device("cuda:0")
    B, h, w, C = 32, 28, 28, 384
    torch.manual_seed(0)
    mha = torch.nn.MultiheadAttention(C, 8, dropout=0.1).to(dev).train()
    qmap = torch.randn(B, C, h, w, device=dev, requires_grad=True)
    feat = torch.randn(B, C, h, w, device=dev)
    gout = torch.randn(B, C, h, w, device=dev)

    def torch_route():                           # DepthGuidance._cross_attend with the flag off
        mha.zero_grad(set_to_none=True)
        qmap.grad = None
        kv = feat.reshape(B, C, -1).permute(2, 0, 1)
        mha(qmap.reshape(B, C, -1).permute(2, 0, 1), kv, kv)[0].permute(1, 2, 0).reshape(B, C, h, w).backward(gout)

    def fused_route():
        mha.zero_grad(set_to_none=True)
        qmap.grad = None
        multihead_cross_attention(mha, qmap, feat, True).backward(gout)

    rows = []
    res = alternate({"torch": torch_route, "fused": fused_route}, a.calls, a.repeats)
    for k, v in res.items():
        rows.append({"what": "_cross_attend forward+backward, one pass, training, p=0.1", "form": k, "B": B, "grid": [h, w], "C": C,
                     "calls": a.calls, "repeats": a.repeats, **v})
    if not a.no_step:
        g = torch.Generator().manual_seed(0)
        batch = {"img": torch.randn(B, 3, 224, 224, generator=g).to(dev), "img_pos": torch.randn(B, 3, 224, 224, generator=g).to(dev),
                 "label": torch.randint(0, 27, (B, 224, 224), generator=g).to(dev),
                 "depth": torch.rand(B, 1, 224, 224, generator=g).to(dev), "depth_pos": torch.rand(B, 1, 224, 224, generator=g).to(dev)}
        segs = {}
        for name, flag in (("step, flag off", False), ("step, flag on", True)):
            torch.manual_seed(1)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                seg = UnsupervisedSegmenter(27, default_segmenter_cfg(arch="dino_depth", guidance="cross_attn",
                                                                      dg_fused_cross_attn=flag)).to(dev).train()
            segs[name] = (lambda s=seg: s.training_step(batch))
        res = alternate(segs, max(a.calls // 4, 3), a.repeats, warmup=2)
        for k, v in res.items():
            rows.append({"what": "dino_depth training_step, guidance cross_attn (stand-in backbone)", "form": k, "B": B, **v})
    with open(a.out, "w") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
