"""The probes' predictions at label resolution and their confusion counts on the GPU (dg_segment_predict through
evaluation.predict_and_score and UnsupervisedSegmenter.validation_step / on_validation_epoch_end / evaluate_batch), against the
reference's order of operations restated on the CPU in fp64: F.interpolate -> 1x1 convolution / F.normalize + einsum -> argmax ->
bincount (src/train_segmentation.py:471-535, src/eval_segmentation.py:146-170 without the CRF).

The kernel takes the arg-maxes of resized fp32 score maps, the reference of scores computed on the resized code: the two orders
agree exactly except where a pixel's two best scores are closer than the arithmetic's rounding.  Such a pixel (reference top-2
margin <= 1e-5 * (1 + |top1|)) may differ; at most 1e-4 of the pixels (at least one) may, and every matrix entry may then move by
at most two per differing pixel.  The kernel's own matrices must equal ops.confusion_update of its own predictions exactly."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def ref_chain(code, label, lin_w, lin_b, clusters, code_flip=None, same=((), ())):
    """fp64 restatement of the reference on the CPU: (preds_lin, preds_clu, near_lin, near_clu) over (B, H, W).  same: pairs (i, j)
    of duplicated linear rows / centres whose score j is set to score i (the CPU convolution and einsum block their output
    channels and need not round two equal rows alike)."""
    c = code.detach().cpu().double()
    if code_flip is not None:
        c = (c + code_flip.detach().cpu().double().flip(dims=[3])) / 2
    H, W = label.shape[-2:]
    n = lin_w.shape[0]
    wl = lin_w.detach().cpu().double().reshape(n, -1, 1, 1)
    bl = lin_b.detach().cpu().double() if lin_b is not None else None
    cn = F.normalize(clusters.detach().cpu().double(), dim=1)
    outs = [[], [], [], []]
    for b in range(c.shape[0]):                                    # one image at a time (D = 384 maps at label resolution)
        up = F.interpolate(c[b:b + 1], (H, W), mode="bilinear", align_corners=False)
        for i, s in enumerate((F.conv2d(up, wl, bl), torch.einsum("bchw,nc->bnhw", F.normalize(up, dim=1), cn))):
            for src, dst in same[i]:
                s[:, dst] = s[:, src]
            outs[i].append(s.argmax(1)[0])
            if s.shape[1] > 1:
                top = s.topk(2, dim=1).values[0]
                outs[2 + i].append((top[0] - top[1]) <= 1e-5 * (1 + top[0].abs()))
            else:
                outs[2 + i].append(torch.zeros(H, W, dtype=torch.bool))
    return tuple(torch.stack(o) for o in outs)


def counts(pred, label, rows, n):
    p, a = pred.reshape(-1).cpu().long(), label.reshape(-1).cpu().long()
    ok = (a >= 0) & (a < n) & (p >= 0) & (p < n)
    return torch.bincount(p[ok] * n + a[ok], minlength=rows * n).reshape(rows, n)


def check_against_ref(got, want, near, stats, want_stats):
    """got/want (B,H,W) predictions, near the reference's near-tie pixels; stats / want_stats the two matrices."""
    got = got.cpu()
    diff = got != want
    assert not (diff & ~near).any(), f"{int((diff & ~near).sum())} pixels differ away from a near-tie"
    nd = int(diff.sum())
    assert nd <= max(1, int(1e-4 * diff.numel())), (nd, diff.numel())
    assert int((stats.cpu() - want_stats).abs().sum()) <= 2 * nd
    return nd


def make_probes(lin_w, lin_b, clusters):
    from depthg_amd.head import ClusterLookup
    n, D = lin_w.shape
    linear = torch.nn.Conv2d(D, n, (1, 1)).to(DEV)
    cluster = ClusterLookup(D, clusters.shape[0]).to(DEV)
    with torch.no_grad():
        linear.weight.copy_(lin_w.reshape(n, D, 1, 1))
        linear.bias.copy_(lin_b)
        cluster.clusters.copy_(clusters)
    return linear, cluster


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fixture_predictions_and_stats_are_exact(case):
    from depthg_amd import predict_and_score
    from depthg_amd.metrics import UnsupervisedMetrics
    g = load_golden("eval.npz")
    B, D, h, w, H, W, n, e, flip, _ = (int(v) for v in g[f"{case}_cfg"])
    t = lambda k: torch.from_numpy(g[f"{case}_{k}"]).to(DEV)          # noqa: E731
    linear, cluster = make_probes(t("lin_w"), t("lin_b"), t("clusters"))
    lm, cm = UnsupervisedMetrics("test/linear/", n, 0, False), UnsupervisedMetrics("test/cluster/", n, e, True)
    label = t("label").long()
    lp, cp = predict_and_score(t("code"), label, linear, cluster, lm, cm, code_flip=t("code_flip") if flip else None, n_store=B)
    torch.cuda.synchronize()
    assert torch.equal(lp.cpu(), torch.from_numpy(g[f"{case}_linear_preds"]).long())
    assert torch.equal(cp.cpu(), torch.from_numpy(g[f"{case}_cluster_preds"]).long())
    assert lm.stats.is_cuda and np.array_equal(lm.stats.cpu().numpy(), g[f"{case}_stats_lin"])
    assert np.array_equal(cm.stats.cpu().numpy(), g[f"{case}_stats_clu"])


def _sweep_cases(count=30):
    rng = np.random.default_rng(2024)
    cases = []
    for i in range(count):
        B = int(rng.integers(1, 5))
        D = int(rng.choice([3, 27, 70, 100, 384]))
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        mode = ["equal", "up", "down", "ratio"][i % 4]
        if mode == "equal":
            H, W = h, w
        elif mode == "up":
            k = int(rng.integers(2, 5))
            H, W = min(h * k, 120), min(w * k, 120)
        elif mode == "down":
            H, W = max(1, h // 2), max(1, (w * 2) // 3)
        else:
            H, W = int(rng.integers(1, 121)), int(rng.integers(1, 121))
        n, e = int(rng.integers(1, 41)), int(rng.integers(0, 6))
        cases.append((B, D, h, w, H, W, n, e, bool(i % 3 == 1), int(rng.integers(0, 1 << 30))))
    return cases


SWEEP = _sweep_cases()


def _draw(B, D, h, w, H, W, n, e, flip, seed):
    g = torch.Generator().manual_seed(seed)
    code = torch.randn(B, D, h, w, generator=g)
    code_flip = torch.randn(B, D, h, w, generator=g) if flip else None
    lin_w = torch.randn(n, D, generator=g) / D ** 0.5
    lin_b = torch.randn(n, generator=g) * 0.1
    clusters = torch.randn(n + e, D, generator=g)
    label = torch.randint(-1, n + 1, (B, H, W), generator=g)
    label[torch.rand(B, H, W, generator=g) < 0.05] = 255
    return code, code_flip, lin_w, lin_b, clusters, label


def _run(code, code_flip, lin_w, lin_b, clusters, label, n_store=None):
    from depthg_amd import ops
    n, m = lin_w.shape[0], clusters.shape[0]
    sl = torch.zeros(n, n, dtype=torch.int64, device=DEV)
    sc = torch.zeros(m, n, dtype=torch.int64, device=DEV)
    d = lambda t: t.to(DEV) if t is not None else None                  # noqa: E731
    lp, cp = ops.segment_predict(d(code), d(label), d(lin_w), d(lin_b), d(clusters), code_flip=d(code_flip), stats_lin=sl,
                                 stats_clu=sc, n_store=code.shape[0] if n_store is None else n_store)
    return lp, cp, sl, sc


@pytest.mark.parametrize("case", SWEEP, ids=[f"B{c[0]}D{c[1]}_{c[2]}x{c[3]}to{c[4]}x{c[5]}_n{c[6]}e{c[7]}{'_flip' if c[8] else ''}" for c in SWEEP])
def test_random_sweep_against_reference_order(case):
    from depthg_amd import ops
    B, D, h, w, H, W, n, e, flip, seed = case
    code, code_flip, lin_w, lin_b, clusters, label = _draw(*case)
    lp, cp, sl, sc = _run(code, code_flip, lin_w, lin_b, clusters, label)
    rl, rc, nl, nc = ref_chain(code, label, lin_w, lin_b, clusters, code_flip)
    check_against_ref(lp, rl, nl, sl, counts(rl, label, n, n))
    check_against_ref(cp, rc, nc, sc, counts(rc, label, n + e, n))
    # the kernel's matrices are exactly the counts of its own predictions
    for preds, st, extra in ((lp, sl, 0), (cp, sc, n + e - n)):
        own = torch.zeros_like(st)
        ops.confusion_update(own, preds, label.to(DEV), n, extra)
        assert torch.equal(own, st)


def test_exact_ties_go_to_the_lowest_index():
    B, D, h, w, H, W, n, e = 2, 16, 7, 9, 30, 41, 6, 3
    g = torch.Generator().manual_seed(7)
    code = torch.randn(B, D, h, w, generator=g)
    code[1] = 0.0                                                   # an all-zero code map: every similarity 0, logits = bias
    lin_w = torch.randn(n, D, generator=g)
    lin_b = torch.tensor([0.1, 0.5, -0.3, 0.2, 0.5, -0.1])
    lin_w[4] = lin_w[1]                                              # duplicated linear row (weights and bias)
    clusters = torch.randn(n + e, D, generator=g)
    clusters[5] = clusters[2]                                        # duplicated centre
    clusters[0] = 0.0                                                # a zero centre: similarity 0 everywhere
    label = torch.randint(0, n, (B, H, W), generator=g)
    lp, cp, sl, sc = _run(code, None, lin_w, lin_b, clusters, label)
    rl, rc, nl, nc = ref_chain(code, label, lin_w, lin_b, clusters, same=(((1, 4),), ((2, 5),)))
    lp, cp = lp.cpu(), cp.cpu()
    assert (lp != 4).all() and (cp != 5).all()                         # the later duplicates never win
    assert torch.equal(lp[1], torch.full((H, W), 1)) and torch.equal(cp[1], torch.zeros(H, W, dtype=torch.long))
    assert torch.equal(rl[1], lp[1]) and torch.equal(rc[1], cp[1])     # torch.argmax on the CPU: the same first maxima
    assert (cp[0] == 2).any()                                          # the duplicated centre does win somewhere
    check_against_ref(lp, rl, nl, sl, counts(rl, label, n, n))
    check_against_ref(cp, rc, nc, sc, counts(rc, label, n + e, n))


def test_n_store_writes_only_the_first_images():
    from depthg_amd import _lib
    from depthg_amd.ops import _ptr, _stream
    B, D, h, w, H, W, n, e = 4, 27, 10, 12, 40, 48, 9, 2
    code, _, lin_w, lin_b, clusters, label = (t.to(DEV) if t is not None else None for t in _draw(B, D, h, w, H, W, n, e, False, 5))
    full_l, full_c, _, _ = _run(code, None, lin_w, lin_b, clusters, label)
    kp = (n + 3) // 4 * 4 + (n + e + 3) // 4 * 4
    scratch = torch.empty(B * h * w * kp * 4, dtype=torch.uint8, device=DEV)
    pl = torch.full((B, H, W), -7, dtype=torch.int64, device=DEV)
    pc = torch.full((B, H, W), -7, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    rc = lib.dg_segment_predict(_ptr(code), None, B, D, h, w, _ptr(lin_w), _ptr(lin_b), n, _ptr(clusters), n + e, _ptr(label), H, W,
                                None, None, 2, _ptr(pl), _ptr(pc), _ptr(scratch), scratch.numel(), _stream(DEV))
    _lib.check(rc, "dg_segment_predict")
    torch.cuda.synchronize()
    assert torch.equal(pl[:2], full_l[:2]) and torch.equal(pc[:2], full_c[:2])
    assert (pl[2:] == -7).all() and (pc[2:] == -7).all()
    lp, cp, _, _ = _run(code, None, lin_w, lin_b, clusters, label, n_store=0)
    assert lp is None and cp is None


def test_calls_accumulate_and_repeat_bit_for_bit():
    from depthg_amd import predict_and_score
    from depthg_amd.metrics import UnsupervisedMetrics
    B, D, h, w, H, W, n, e = 3, 70, 20, 20, 160, 160, 27, 3
    code, code_flip, lin_w, lin_b, clusters, label = (t.to(DEV) for t in _draw(B, D, h, w, H, W, n, e, True, 11))
    linear, cluster = make_probes(lin_w, lin_b, clusters)
    runs = []
    for _ in range(3):
        lm, cm = UnsupervisedMetrics("l/", n, 0, False), UnsupervisedMetrics("c/", n, e, True)
        predict_and_score(code, label, linear, cluster, lm, cm, code_flip=code_flip)
        once = (lm.stats.clone(), cm.stats.clone())
        predict_and_score(code, label, linear, cluster, lm, cm, code_flip=code_flip)
        assert torch.equal(lm.stats, 2 * once[0]) and torch.equal(cm.stats, 2 * once[1])
        assert int(once[0].sum()) == int(((label >= 0) & (label < n)).sum())
        runs.append((lm.stats.cpu(), cm.stats.cpu()))
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])


def _val_batch(B, g, hw_img=112, n_classes=27):
    return {"img": torch.randn(B, 3, hw_img, hw_img, generator=g).to(DEV),
            "img_pos": torch.randn(B, 3, hw_img, hw_img, generator=g).to(DEV),
            "label": torch.randint(-1, n_classes, (B, hw_img, hw_img), generator=g).to(DEV),
            "depth": torch.randint(1, 256, (B, 1, hw_img, hw_img), generator=g).float().to(DEV),
            "depth_pos": torch.randint(1, 256, (B, 1, hw_img, hw_img), generator=g).float().to(DEV)}


def _eval_code(m, img):
    was = m.net.training
    m.net.eval()
    with torch.no_grad():
        code = m.net(img)[1]
    m.net.train(was)
    return code


def test_validation_step_and_epoch_end():
    from depthg_amd.metrics import UnsupervisedMetrics
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(4)
    cfg = default_segmenter_cfg(dim=70, extra_clusters=3, dg_outputs="reduced")
    m = UnsupervisedSegmenter(27, cfg).to(DEV)
    m.train()
    g = torch.Generator().manual_seed(21)
    epochs = []
    for epoch in range(2):
        want_l, want_c = torch.zeros(27, 27, dtype=torch.int64), torch.zeros(30, 27, dtype=torch.int64)
        nd = 0
        for step in range(2):
            batch = _val_batch(6, g)
            out = m.validation_step(batch, step)
            assert m.net.training                                          # the mode it found
            assert set(out) == {"img", "linear_preds", "cluster_preds", "label"} and len(m.validation_step_outputs) == step + 1
            assert all(v.device.type == "cpu" for v in out.values())
            assert out["img"].shape == (5, 3, 112, 112) and out["label"].shape == (5, 112, 112)
            assert out["linear_preds"].shape == (5, 112, 112) and out["cluster_preds"].shape == (5, 112, 112)
            code = _eval_code(m, batch["img"])
            rl, rc, nl, nc = ref_chain(code, batch["label"], m.linear_probe.weight, m.linear_probe.bias, m.cluster_probe.clusters)
            assert not ((out["linear_preds"] != rl[:5]) & ~nl[:5]).any() and not ((out["cluster_preds"] != rc[:5]) & ~nc[:5]).any()
            want_l += counts(rl, batch["label"], 27, 27)
            want_c += counts(rc, batch["label"], 30, 27)
            nd += int(nl.sum()) + int(nc.sum())                        # pixels allowed to differ
        got_l, got_c = m.linear_metrics.stats.cpu().clone(), m.cluster_metrics.stats.cpu().clone()
        assert int((got_l - want_l).abs().sum()) <= 2 * nd and int((got_c - want_c).abs().sum()) <= 2 * nd
        ref_l, ref_c = UnsupervisedMetrics("test/linear/", 27, 0, False), UnsupervisedMetrics("test/cluster/", 27, 3, True)
        ref_l.stats, ref_c.stats = want_l, want_c
        want = {**ref_l.compute(), **ref_c.compute()}
        res = m.on_validation_epoch_end()
        tol = 0 if (torch.equal(got_l, want_l) and torch.equal(got_c, want_c)) else 0.5
        for k, v in want.items():
            assert abs(res[k] - v) <= tol, (k, res[k], v)
        assert int(m.linear_metrics.stats.abs().sum()) == 0 and int(m.cluster_metrics.stats.abs().sum()) == 0
        assert m.validation_step_outputs == []
        epochs.append(res)
    for key in ("cluster/Accuracy", "cluster/mIoU", "linear/Accuracy", "linear/mIoU"):
        head, name = key.split("/")
        assert epochs[1][f"test/{head}/Max{name}"] == max(epochs[0][f"test/{key}"], epochs[1][f"test/{key}"])
        assert epochs[0][f"test/{head}/Max{name}"] == epochs[0][f"test/{key}"]
    assert m.max_cluster_miou == epochs[1]["test/cluster/MaxmIoU"]
    # a training step right after a validation step sees the training-mode featurizer
    loss, _ = m.training_step(_val_batch(2, g), 0)
    assert torch.isfinite(loss)


def test_evaluate_batch_with_flip():
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(6)
    cfg = default_segmenter_cfg(dim=70, extra_clusters=2)
    m = UnsupervisedSegmenter(27, cfg).to(DEV)
    m.eval()
    g = torch.Generator().manual_seed(8)
    batch = _val_batch(4, g)
    lp, cp = m.evaluate_batch(batch, flip=True)
    assert not m.net.training and lp.shape == (4, 112, 112) and cp.shape == (4, 112, 112)
    code1 = _eval_code(m, batch["img"])
    code2 = _eval_code(m, batch["img"].flip(dims=[3]))
    rl, rc, nl, nc = ref_chain(code1, batch["label"], m.linear_probe.weight, m.linear_probe.bias, m.cluster_probe.clusters, code2)
    check_against_ref(lp, rl, nl, m.test_linear_metrics.stats, counts(rl, batch["label"], 27, 27))
    check_against_ref(cp, rc, nc, m.test_cluster_metrics.stats, counts(rc, batch["label"], 29, 27))
    assert m.test_cluster_metrics.compute()["final/cluster/Accuracy"] >= 0.0
