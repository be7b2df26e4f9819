"""Times both probes of the training step, forward plus backward, through the unfused route against the fused one.

    python scripts/probe_step_time.py [--out profiles/probe_step_time.jsonl] [--repeats 5] [--calls 20]

B = 32, D = 70, n = 27 classes and centres, a 28 x 28 code, 224 x 224 labels (a tenth unlabelled).  Two forms in one process,
alternated inside each of `--repeats` repeats, `--calls` calls per sample, host clock between two device synchronisations:
    a_unfused   linear_probe(code.detach().clone()), head.probe_cross_entropy, ClusterLookup(code, None), (lin + clu).backward()
    b_fused     head.fused_probe_losses(code.detach(), ...), (lin + clu).backward()                     (cfg.dg_fused_probes)
One JSON line per form: microseconds per call, median [min, max] over the repeats.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "probe_step_time.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    from depthg_amd.head import ClusterLookup, fused_probe_losses, probe_cross_entropy
    dev = torch.device("cuda:0")
    B, D, n, hw, HW = 32, 70, 27, 28, 224
    torch.manual_seed(0)
    code = torch.randn(B, D, hw, hw, device=dev, requires_grad=True) * 1.0          # attached, as the step's code is
    label = torch.randint(0, n, (B, HW, HW), device=dev)
    label[torch.rand(B, HW, HW, device=dev) < 0.1] = -1
    linear = torch.nn.Conv2d(D, n, (1, 1)).to(dev)
    cluster = ClusterLookup(D, n).to(dev)
    params = list(linear.parameters()) + list(cluster.parameters())

    def zero():
        for p in params:
            p.grad = None

    def unfused():
        zero()
        detached = code.detach().clone()
        lin = probe_cross_entropy(linear(detached), label)
        clu, _ = cluster(detached, None)
        (lin + clu).backward()

    def fused():
        zero()
        lin, clu = fused_probe_losses(code.detach(), label, linear.weight, linear.bias, cluster.clusters)
        (lin + clu).backward()

    forms = {"a_unfused": unfused, "b_fused": fused}
    grads = {}
    for name, fn in forms.items():              # warm-up: allocator, kernel attributes, clocks - and the two routes' gradients
        timed(fn, args.calls)
        grads[name] = [p.grad.clone() for p in params]
    agree = [float((a - b).norm() / a.norm()) for a, b in zip(grads["a_unfused"], grads["b_fused"])]
    samples = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, fn in forms.items():
            samples[name].append(timed(fn, args.calls))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for name, us in samples.items():
            us = sorted(us)
            line = {"form": name, "unit": "microseconds per call (forward + backward)", "median": round(statistics.median(us), 1),
                    "min": round(us[0], 1), "max": round(us[-1], 1), "repeats": args.repeats, "calls_per_sample": args.calls,
                    "shape": {"B": B, "D": D, "n": n, "code": [hw, hw], "label": [HW, HW]},
                    "gradients_rel_l2_between_forms": [float(f"{v:.3e}") for v in agree], "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
