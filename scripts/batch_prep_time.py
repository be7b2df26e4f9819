#!/usr/bin/env python3
"""Time three routes to one prepared training batch on the MI355X - B = 32 samples plus their 32 positives from decoded 500 x 375
sources to 224 x 224 (centre crop), image, label and depth each - one JSON line per form into profiles/batch_prep_time.jsonl:

    host     the reference's chain per sample on the host (PIL nearest resize and crop, ToTensor, Normalize, ToTargetTensor;
             data.prepare_samples on the CPU, spread over 16 threads), then the upload of the float32 / int64 results
    fused    the raw planes packed into one pinned buffer, its upload, the table upload and dg_batch_prep (data.prepare_samples on the GPU)
    launch   dg_batch_prep alone: the planes and the tables already on the GPU

Decoding is outside all three (the same for each).  Host clock around `--steps` calls ending in a device synchronise, after warm-up;
the forms alternate in one process and each is repeated `--repeats` times: median, minimum and maximum of the repeats are on the line
(microseconds per call).  `--only launch --steps N --repeats 1` is the program for a kernel trace.  Needs the GPU.

    python scripts/batch_prep_time.py [--steps 20] [--repeats 5] [--warmup 3] [--out profiles/batch_prep_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from depthg_amd import data, ops  # noqa: E402

HOST_THREADS = 16


def clock(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def spread(ts):
    return {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2), "repeats": len(ts)}


class _Planes:
    """What prepare_samples asks of a dataset: CroppedDataset's label offset and mask rule."""
    label_offset, mask_rule, has_labels, label_dims = -1, ops.BATCH_MASK_BOOL_IGNORED, True, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["host", "fused", "launch"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_prep_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("batch_prep_time.py: needs the GPU")
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)                                   # (the host form's parallelism is its 16 sample threads)
    B, sw, sh, res = 32, 500, 375, 224
    rng = np.random.default_rng(0)
    samples = [data.Sample(rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8), rng.integers(0, 28, (sh, sw), dtype=np.uint8),
                           rng.integers(0, 256, (sh, sw), dtype=np.uint8)) for _ in range(2 * B)]
    ds = _Planes()
    pool = ThreadPoolExecutor(max_workers=HOST_THREADS)
    last = {}

    def host():
        rows = list(pool.map(lambda s: data._cpu_chain(ds, s, res, "center", None, True), samples))
        last["host"] = tuple(torch.stack([r[k] for r in rows]).to(dev, non_blocking=True) for k in range(4))

    def fused():
        last["fused"] = data.prepare_samples(ds, samples, res, "center", dev, True)

    tables = [data.loader_index_tables(sw, sh, res, "center")[:2] for _ in samples]
    packed, records, table = data.pack_batch(ds, samples, tables, (res, res), True)
    packed_dev = packed.to(dev)
    params_dev = torch.cat([records.reshape(-1), table.reshape(-1)]).to(dev)

    def launch():
        last["launch"] = ops.batch_prep(packed_dev, records, table, (res, res), device=dev, params=params_dev)

    forms = {"host": host, "fused": fused, "launch": launch}
    if args.only:
        forms = {args.only: forms[args.only]}
    for f in forms.values():
        clock(f, args.warmup)
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, f in forms.items():
            times[k].append(clock(f, args.steps))
    extra = {}
    if "host" in last and "fused" in last:
        extra["img_bits_equal"] = bool(torch.equal(last["host"][0].view(torch.int32), last["fused"][0].view(torch.int32)))
        extra["label_mask_depth_equal"] = all(bool(torch.equal(a, b)) for a, b in zip(last["host"][1:], last["fused"][1:]))
    n_out = 2 * B * res * res
    moved = {"source_bytes": int(packed.numel()), "written_bytes": n_out * (12 + 8 + 1 + 4), "table_bytes": int(params_dev.numel() * 4)}
    lines = []
    for k, ts in times.items():
        rec = {"form": k, "shape": f"B={B}+{B}, {sw}x{sh} uint8 sources (image, label, depth) -> {res}x{res}, centre crop",
               "steps": args.steps, **spread(ts), **moved, **extra}
        if "host" in times:
            rec["vs_host"] = round(statistics.median(ts) / statistics.median(times["host"]), 5)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    pool.shutdown()


if __name__ == "__main__":
    main()
