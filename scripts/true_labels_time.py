"""Time what cfg.use_true_labels adds to a step at the headline batch: B = 32 + 32 label maps of 224 x 224, K = n_classes + 1 = 28.
Host clock around 20 calls, five alternated repeats per form, median [min, max] in microseconds per call:
    (a) the reference's torch chain on the device for both maps: F.one_hot(label + 1, K).permute(0, 3, 1, 2).float(), twice
    (b) ops.label_onehot(label, n_classes, label_pos): one launch, both maps
    (c) ops.fps_coords_large_pair at the labels' resolution (224 x 224, S = 11) - 121 sequential rounds over 50 176 points per image
    (d) ops.fps_coords_pair on the 28 x 28 grid of the unsupervised step, for scale
    (e) the reference's sample() on the device for the seven signal operands of a step (anchors, positives, five negatives through
        their batch maps: orig_feats[perm], then F.grid_sample of the whole map, src/modules.py:822-825, 1340-1345), S = 11
    (f) ops.sample_rows (bf16 rows, the loss's feature operand) for the same seven operands: the taps read in place
    (g, h) the whole loss call, forward and backward, on the 224 x 224 signal over 28 x 28 code maps of 70 channels, depth_sampling
        "none" and "fps"
    (i, j, k) training_step (forward, backward and the optimisers' steps) of the stand-in model at 224 x 224 with the key on ("none",
        "fps") and, for scale, the unsupervised step of the same model ("fps"); cfg.fps_sample_decay off, so that S stays 11
(b) is also stated as bytes moved per second (labels read once, the signal written once); (f) as the bytes of the taps it reads and
the rows it writes per second - useful bytes: every 4-byte tap costs a whole cache line's sector, so this is far below a copy's rate.
Appends one JSON line per form to profiles/true_labels_time.jsonl.

    python scripts/true_labels_time.py [--out profiles/true_labels_time.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from depthg_amd import ContrastiveCorrelationLoss, ops  # noqa: E402
from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg  # noqa: E402

B, N_CLASSES, HW, S, GRID, CALLS, REPEATS, N_NEG = 32, 27, 224, 11, 28, 20, 5, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_labels_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    label, label_pos = (torch.randint(-1, N_CLASSES, (B, HW, HW), generator=g).to(dev) for _ in range(2))
    depth, depth_pos = (torch.rand(B, 1, HW, HW, generator=g).to(dev) * 255 + 1 for _ in range(2))
    K = N_CLASSES + 1
    chain = lambda t: F.one_hot(t + 1, K).permute(0, 3, 1, 2).to(torch.float32)
    forms = {"a_torch_chain_both_maps": lambda: (chain(label), chain(label_pos)),
             "b_label_onehot_pair": lambda: ops.label_onehot(label, N_CLASSES, label_pos, check=False),
             "c_fps_coords_large_pair_224": lambda: ops.fps_coords_large_pair(depth, depth_pos, (HW, HW), S),
             "d_fps_coords_pair_28": lambda: ops.fps_coords_pair(depth, depth_pos, (GRID, GRID), S)}
    # ---- the sampling alone: the seven signal operands of a step
    signal, signal_pos = ops.label_onehot(label, N_CLASSES, label_pos, check=False)
    coords1, coords2 = (torch.rand(B, S, S, 2, generator=g).to(dev) * 2 - 1 for _ in range(2))
    perms = torch.stack([torch.randperm(B, generator=g) for _ in range(N_NEG)]).to(dev)
    ref_sample = lambda t, c: F.grid_sample(t, c.permute(0, 2, 1, 3), padding_mode="border", align_corners=True)

    def reference_sampling():
        return [ref_sample(signal, coords1), ref_sample(signal_pos, coords2)] + [ref_sample(signal[perms[k]], coords2) for k in range(N_NEG)]

    def direct_sampling():
        return [ops.sample_rows(signal, coords1, bf16=True), ops.sample_rows(signal_pos, coords2, bf16=True)] + \
            [ops.sample_rows(signal, coords2, perms[k], bf16=True) for k in range(N_NEG)]

    for r, d in zip(reference_sampling(), direct_sampling()):          # the same values, as rows
        want = r.permute(0, 2, 3, 1).reshape(B, S * S, K)
        assert float((d[..., :K].float() - want).abs().max()) <= 2.0 ** -8 + 1e-6 and not bool(d[..., K:].any())
    forms["e_grid_sample_7_operands"] = reference_sampling
    forms["f_sample_rows_7_operands"] = direct_sampling
    sample_bytes = (2 + N_NEG) * B * S * S * (K * 4 * 4 + 128 * 2)

    # ---- the whole loss call and the whole step
    code, code_pos = (torch.randn(B, 70, GRID, GRID, generator=g).to(dev).requires_grad_(True) for _ in range(2))

    def loss_call(sampling):
        loss = ContrastiveCorrelationLoss(default_segmenter_cfg(depth_sampling=sampling, neg_samples=N_NEG, feature_samples=S))

        def run():
            loss(signal, signal_pos, None, None, code, code_pos, depth, depth_pos)
            loss.total.backward()
        return run

    forms["g_loss_call_224_none"] = loss_call("none")
    forms["h_loss_call_224_fps"] = loss_call("fps")
    batch = {"img": torch.randn(B, 3, HW, HW, generator=g).to(dev), "img_pos": torch.randn(B, 3, HW, HW, generator=g).to(dev),
             "label": label, "label_pos": label_pos, "depth": depth, "depth_pos": depth_pos}

    def step(**over):
        torch.manual_seed(0)
        cfg = default_segmenter_cfg(neg_samples=N_NEG, feature_samples=S, fps_sample_decay=False, **over)
        seg = UnsupervisedSegmenter(N_CLASSES, cfg).to(dev).train()
        return lambda: seg.training_step(batch)

    forms["i_step_true_labels_none"] = step(use_true_labels=True, depth_sampling="none")
    forms["j_step_true_labels_fps"] = step(use_true_labels=True, depth_sampling="fps")
    forms["k_step_unsupervised_fps"] = step(use_true_labels=False, depth_sampling="fps")
    a, b = forms["a_torch_chain_both_maps"](), forms["b_label_onehot_pair"]()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    del a, b
    onehot_bytes = 2 * B * HW * HW * (8 + 4 * K)
    times = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / CALLS * 1e6)
    with open(args.out, "a") as fh:
        for name, ts in times.items():
            line = dict(form=name, B=f"{B}+{B}", K=K, label_hw=HW, S=S, calls=CALLS, repeats=REPEATS, us_median=round(statistics.median(ts), 1),
                        us_min=round(min(ts), 1), us_max=round(max(ts), 1), device=torch.cuda.get_device_name(0))
            if name == "b_label_onehot_pair":
                line.update(bytes=onehot_bytes, tb_per_s_at_median=round(onehot_bytes / statistics.median(ts) / 1e6, 3))
            if name == "f_sample_rows_7_operands":
                line.update(useful_bytes=sample_bytes, tb_per_s_at_median=round(sample_bytes / statistics.median(ts) / 1e6, 4))
            print(json.dumps(line))
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
