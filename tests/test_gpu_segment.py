"""Label-free inference on the GPU (dg_segment_labels / dg_label_paint through ops.segment_labels, ops.label_paint,
evaluation.segment and UnsupervisedSegmenter.segment): the byte label maps against the scored route's predictions (bit for bit) and
against the reference's order of operations in fp64 (tests/test_gpu_eval.py's rule: only a near-tie pixel may differ, at most 1e-4 of
the pixels and at least one), the remap, the paint, the CRF route, determinism and coverage.

Shapes (B, D, h, w, H, W, n, m): the smallest at which the kernel's chunking can go wrong - one chunk for many CUs (7 and 39 label
rows), eight chunks of ten rows with a short last one (74 rows of 50 pixels: chunk starts at every 16-byte phase that 500 bytes
reach), no W a multiple of 4.  The reference chain of each case is computed once."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_eval import make_probes, ref_chain

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = [(1, 5, 3, 4, 7, 9, 3, 3), (3, 70, 5, 5, 13, 11, 27, 30), (2, 16, 28, 28, 37, 50, 27, 27)]
IDS = [f"B{c[0]}D{c[1]}_{c[2]}x{c[3]}to{c[4]}x{c[5]}_n{c[6]}m{c[7]}" for c in CASES]
SEEDS = {CASES[0]: 101, CASES[1]: 102, CASES[2]: 103}


@functools.lru_cache(maxsize=None)
def draw(case):
    """Seeded continuous inputs of a case (CPU tensors; nobody writes to them) and normalised images of random bytes."""
    from depthg_amd import ops
    B, D, h, w, H, W, n, m = case
    g = torch.Generator().manual_seed(SEEDS[case])
    code, code_flip = torch.randn(B, D, h, w, generator=g), torch.randn(B, D, h, w, generator=g)
    lin_w, lin_b, clusters = torch.randn(n, D, generator=g) / D ** 0.5, torch.randn(n, generator=g) * 0.1, torch.randn(m, D, generator=g)
    raw = torch.randint(0, 256, (B, 3, H, W), generator=g)
    mean, std = (torch.tensor(v).reshape(1, 3, 1, 1) for v in (ops.IMAGENET_MEAN, ops.IMAGENET_STD))
    img = (raw.float() / 255 - mean) / std
    return code, code_flip, lin_w, lin_b, clusters, img, raw


@functools.lru_cache(maxsize=None)
def reference(case, flip):
    """(preds_lin, preds_clu, near_lin, near_clu) of the fp64 chain, once per case."""
    code, code_flip, lin_w, lin_b, clusters, _, _ = draw(case)
    B, _, _, _, H, W, _, _ = case
    return ref_chain(code, torch.zeros(B, H, W), lin_w, lin_b, clusters, code_flip if flip else None)


def d(t):
    return t.to(DEV) if t is not None else None


def labels(case, flip, **kw):
    from depthg_amd import ops
    code, code_flip, lin_w, lin_b, clusters, _, _ = draw(case)
    return ops.segment_labels(d(code), d(lin_w), d(lin_b), d(clusters), case[4], case[5], code_flip=d(code_flip) if flip else None, **kw)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_labels_are_the_scored_routes_bits_and_the_references_order(case, flip):
    from depthg_amd import ops
    code, code_flip, lin_w, lin_b, clusters, _, _ = draw(case)
    B, _, _, _, H, W, n, m = case
    out = labels(case, flip)
    assert set(out) == {"lin", "clu"}
    for t in out.values():
        assert t.dtype == torch.uint8 and tuple(t.shape) == (B, H, W) and t.is_cuda
    label = torch.zeros(B, H, W, dtype=torch.int64, device=DEV)
    lp, cp = ops.segment_predict(d(code), label, d(lin_w), d(lin_b), d(clusters), code_flip=d(code_flip) if flip else None, n_store=B)
    assert torch.equal(out["lin"], lp.to(torch.uint8)) and torch.equal(out["clu"], cp.to(torch.uint8))
    rl, rc, nl, nc = reference(case, flip)
    for got, want, near in ((out["lin"], rl, nl), (out["clu"], rc, nc)):
        diff = got.cpu().long() != want
        print(f"{case} flip={flip}: {int(diff.sum())} of {diff.numel()} pixels differ, {int(near.sum())} near-ties in the reference")
        assert not (diff & ~near).any(), f"{int((diff & ~near).sum())} pixels differ away from a near-tie"
        assert int(diff.sum()) <= max(1, int(1e-4 * diff.numel())), (int(diff.sum()), diff.numel())


@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_remap_is_a_table_lookup(case):
    B, _, _, _, H, W, n, m = case
    raw = labels(case, True)["clu"].long()
    g = torch.Generator().manual_seed(7)
    perm = torch.randperm(m, generator=g)
    tables = [perm]
    if m > n:                                             # the Hungarian table of m > n clusters: the unmatched ones are -1
        t = torch.full((m,), -1, dtype=torch.int64)
        t[perm[:n]] = torch.arange(n)
        tables.append(t)
    else:
        t = perm.clone()
        t[perm[:3]] = -1
        tables.append(t)
    for table in tables:
        for remap in (table, table.to(torch.int32).to(DEV), table.tolist()):
            got = labels(case, True, remap=remap)
            mapped = table.to(DEV)[raw]
            assert torch.equal(got["clu"].long(), torch.where(mapped < 0, torch.full_like(mapped, 255), mapped))
            assert torch.equal(got["lin"].long(), labels(case, True)["lin"].long())
    assert (labels(case, True, remap=tables[1])["clu"] == 255).any()


def _restated_paint(a, cmap, lab, pix):
    """(a cmap[label] + (256 - a) pix + 128) >> 8 in fp64, floor of the exact quotient"""
    return torch.floor((a * cmap[lab].double() + (256 - a) * pix.double() + 128) / 256)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_paint(case):
    from depthg_amd import ops
    _, _, _, _, _, img, raw = draw(case)
    B, _, _, _, H, W, n, m = case
    table = (torch.arange(m) - 2).clamp(min=-1)            # two clusters without a class: 255 paints the map's last row
    want4 = ("lin", "clu", "lin_rgb", "clu_rgb")
    cmap = ops.pascal_colormap().long()
    # the de-normalised image in fp64, from the normalised fp32 values the kernel reads
    mean, std = (torch.tensor(v, dtype=torch.float64).reshape(1, 3, 1, 1) for v in (ops.IMAGENET_MEAN, ops.IMAGENET_STD))
    exact = ((img.double() * std + mean) * 255).clamp(0, 255).permute(0, 2, 3, 1)
    assert float((exact - raw.permute(0, 2, 3, 1)).abs().max()) < 1e-3
    base = labels(case, True, remap=table)
    for alpha in (1.0, 0.0, 0.5):
        out = labels(case, True, remap=table, img=None if alpha == 1.0 else d(img), alpha=alpha, want=want4)
        assert torch.equal(out["lin"], base["lin"]) and torch.equal(out["clu"], base["clu"])
        for key, lab in (("lin_rgb", out["lin"]), ("clu_rgb", out["clu"])):
            got = out[key].cpu()
            assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, 3)
            lab = lab.cpu().long()
            if alpha == 1.0:
                assert torch.equal(got.long(), cmap[lab])
            elif alpha == 0.0:
                err = float((got.double() - exact).abs().max())
                print(f"{case} alpha 0: largest distance to the fp64 image {err:.4f} grey levels")
                assert err <= 1.0
            else:
                want = _restated_paint(128, cmap, lab, torch.round(exact))
                err = float((got.double() - want).abs().max())
                print(f"{case} alpha 0.5: largest distance to the restated formula {err:.1f}")
                assert err <= 1.0
    assert (base["clu"] == 255).any()
    # another colour map: its last row for every label past it; mean / std are read
    small = torch.randint(0, 256, (n - 1, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    out = labels(case, True, cmap=small.to(DEV), want=("lin", "lin_rgb"))
    assert torch.equal(out["lin_rgb"].cpu(), small[out["lin"].cpu().long().clamp(max=n - 2)])
    out = labels(case, True, img=d(img), alpha=0.0, want=("lin_rgb",), mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    plain = (img.double() * 255).round().clamp(0, 255).permute(0, 2, 3, 1)
    assert float((out["lin_rgb"].cpu().double() - plain).abs().max()) <= 1.0


def test_crf_route_and_label_paint():
    from depthg_amd import ops, predict_and_score, segment
    case = CASES[1]
    code, code_flip, lin_w, lin_b, clusters, img, _ = draw(case)
    B, _, _, _, H, W, n, m = case
    linear, cluster = make_probes(d(lin_w), d(lin_b), d(clusters))
    label = torch.zeros(B, H, W, dtype=torch.int64, device=DEV)
    pl, pc = predict_and_score(d(code), label, linear, cluster, code_flip=d(code_flip), n_store=B, img=d(img), run_crf=True)

    class Metric:
        assignments = (None, None)
        table = (torch.arange(m) - 3).clamp(min=-1)

        def map_clusters(self, clusters):
            return self.table[clusters]

    seg = segment(d(code), (H, W), linear, cluster, code_flip=d(code_flip), run_crf=True, img=d(img))
    assert torch.equal(seg.linear, pl.to(torch.uint8)) and torch.equal(seg.cluster, pc.to(torch.uint8)) and seg.linear_rgb is None
    seg = segment(d(code), (H, W), linear, cluster, code_flip=d(code_flip), cluster_metrics=Metric(), run_crf=True, img=d(img), overlay=1.0)
    mapped = Metric.table.to(DEV)[pc]
    want_clu = torch.where(mapped < 0, torch.full_like(mapped, 255), mapped)
    assert torch.equal(seg.linear, pl.to(torch.uint8)) and torch.equal(seg.cluster.long(), want_clu)
    cmap = ops.pascal_colormap().long().to(DEV)
    assert torch.equal(seg.linear_rgb.long(), cmap[pl]) and torch.equal(seg.cluster_rgb.long(), cmap[want_clu])
    # without the CRF the same call is the fused route
    plain = segment(d(code), (H, W), linear, cluster, code_flip=d(code_flip), cluster_metrics=Metric())
    assert torch.equal(plain.linear, labels(case, True)["lin"])
    # ops.label_paint alone, on hand-made predictions: 5000 pixels are three chunks, the last one short
    g = torch.Generator().manual_seed(11)
    preds = torch.stack([torch.randint(0, 200, (2, 50, 50), generator=g), torch.randint(0, 40, (2, 50, 50), generator=g)])
    preds[0, 0, 0, :4] = torch.tensor([-1, 254, 255, 1 << 40])           # what no byte label holds becomes 255
    preds[1, 0, 0, :3] = torch.tensor([-1, 40, 39])
    table = torch.randperm(40, generator=g) - 1
    imgp = torch.randn(2, 3, 50, 50, generator=g)
    out = ops.label_paint(preds.to(DEV), remap=table, img=imgp.to(DEV), alpha=0.25, want=("lin", "clu", "lin_rgb", "clu_rgb"))
    want_lin = torch.where((preds[0] < 0) | (preds[0] > 254), torch.full_like(preds[0], 255), preds[0])
    inside = (preds[1] >= 0) & (preds[1] < 40)
    mapped = table[preds[1].clamp(0, 39)]
    want_clu = torch.where(inside & (mapped >= 0), mapped, torch.full_like(mapped, 255))
    assert torch.equal(out["lin"].cpu().long(), want_lin) and torch.equal(out["clu"].cpu().long(), want_clu)
    mean, std = (torch.tensor(v, dtype=torch.float64).reshape(1, 3, 1, 1) for v in (ops.IMAGENET_MEAN, ops.IMAGENET_STD))
    pix = torch.round(((imgp.double() * std + mean) * 255).clamp(0, 255)).permute(0, 2, 3, 1)
    for key, lab in (("lin_rgb", want_lin), ("clu_rgb", want_clu)):
        assert float((out[key].cpu().double() - _restated_paint(64, ops.pascal_colormap().long(), lab, pix)).abs().max()) <= 1.0
    raw = ops.label_paint(preds.to(DEV), m=40, want=("clu",))["clu"].cpu().long()
    assert torch.equal(raw, torch.where(inside, preds[1], torch.full_like(preds[1], 255)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_calls_agree_and_every_requested_byte_is_written(case):
    _, _, _, _, _, img, _ = draw(case)
    B, _, _, _, H, W, n, m = case
    want4 = ("lin", "clu", "lin_rgb", "clu_rgb")
    npx = B * H * W
    sizes = {"lin": npx, "clu": npx, "lin_rgb": 3 * npx, "clu_rgb": 3 * npx}
    shapes = {"lin": (B, H, W), "clu": (B, H, W), "lin_rgb": (B, H, W, 3), "clu_rgb": (B, H, W, 3)}

    def buffers(fill, lead):
        """The four outputs inside guard bytes, each at another 16-byte phase"""
        whole, views = {}, {}
        for i, k in enumerate(want4):
            whole[k] = torch.full((lead + i + sizes[k] + 64,), fill, dtype=torch.uint8, device=DEV)
            views[k] = whole[k][lead + i:lead + i + sizes[k]].view(shapes[k])
        return whole, views

    first = labels(case, True, img=d(img), alpha=0.5, want=want4)
    again = labels(case, True, img=d(img), alpha=0.5, want=want4)
    for k in want4:
        assert torch.equal(first[k], again[k]), k
    for fill, lead in ((0xFF, 0), (0x00, 5), (0xFF, 13)):
        whole, views = buffers(fill, lead)
        out = labels(case, True, img=d(img), alpha=0.5, want=want4, out=views)
        for i, k in enumerate(want4):
            assert out[k].data_ptr() == views[k].data_ptr()
            assert torch.equal(views[k], first[k]), (k, fill, lead)           # every byte written, whatever was there
            guard = torch.cat([whole[k][:lead + i], whole[k][lead + i + sizes[k]:]])
            assert bool((guard == fill).all()), (k, fill, lead)               # and none beside them
    # an output that is not asked for is not touched
    whole, views = buffers(0xFF, 3)
    out = labels(case, True, want=("clu", "lin_rgb"), out=views)
    assert set(out) == {"clu", "lin_rgb"} and torch.equal(out["clu"], first["clu"])
    for k in ("lin", "clu_rgb"):
        assert bool((whole[k] == 0xFF).all()), k


def _batch(B, g, hw=(112, 120)):
    return torch.randn(B, 3, *hw, generator=g).to(DEV)


@pytest.mark.parametrize("arch", ["dino", "dino_depth"])
def test_segmenter_segment_is_evaluate_batchs_path(arch):
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(6)
    kw = dict(arch="dino_depth", guidance="cross_attn") if arch == "dino_depth" else {}
    model = UnsupervisedSegmenter(27, default_segmenter_cfg(dim=70, extra_clusters=2, **kw)).to(DEV)
    model.train()
    g = torch.Generator().manual_seed(8)
    img = _batch(2, g)
    label = torch.randint(0, 27, (2, 112, 120), generator=g).to(DEV)
    seg = model.segment(img)
    assert model.net.training                                                  # the mode it found
    for t in (seg.linear, seg.cluster):
        assert t.dtype == torch.uint8 and tuple(t.shape) == (2, 112, 120) and not t.requires_grad
    lp, cp = model.evaluate_batch({"img": img, "label": label}, flip=True)
    assert torch.equal(seg.linear, lp.to(torch.uint8)) and torch.equal(seg.cluster, cp.to(torch.uint8))
    # evaluate_batch counted: compute() forms the assignment the next call maps the clusters through
    model.test_cluster_metrics.compute()
    table = model.test_cluster_metrics.map_clusters(torch.arange(29)).to(DEV)
    assert int((table < 0).sum()) == 2
    mapped = table[cp]
    seg2 = model.segment(img, overlay=0.5)
    assert torch.equal(seg2.linear, seg.linear)
    assert torch.equal(seg2.cluster.long(), torch.where(mapped < 0, torch.full_like(mapped, 255), mapped))
    assert tuple(seg2.linear_rgb.shape) == (2, 112, 120, 3) and seg2.cluster_rgb.dtype == torch.uint8
    assert torch.equal(model.segment(img, remap=False).cluster, seg.cluster)
    assert torch.equal(model.segment(img, flip=False).linear, model.evaluate_batch({"img": img, "label": label}, flip=False)[0].to(torch.uint8))
