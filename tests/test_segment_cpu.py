"""CPU-side checks of label-free inference (dg_segment_labels / dg_label_paint, ops.segment_labels / ops.label_paint,
evaluation.segment, UnsupervisedSegmenter.segment, depthg_amd.demo): the exports, the refusals before any launch, the default colour
map, the torch route against the reference's chain written out here, and the command line end to end on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

NAMES = ["dg_segment_labels", "dg_label_paint"]


def test_exports_are_declared_bound_and_in_the_library():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "src/demo_segmentation.py:59-78" in header and "src/eval_segmentation.py:170-240" in header
    # the header's order: behind the scored route, in front of the dense CRF
    order = _lib.EXPORTS
    assert order.index("dg_segment_predict") < order.index(NAMES[0]) < order.index(NAMES[1]) < order.index("dg_crf_workspace_bytes")
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 27 and len(_lib.SIGNATURES[NAMES[1]][1]) == 18
    assert lib.dg_version() == _lib.DG_VERSION == 119


P = ctypes.c_void_p(256)                    # a dummy device address: every call below is refused before anything is dereferenced
F3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)


def _labels(B=2, D=8, h=4, w=4, n=3, m=4, H=8, W=8, remap=None, img=None, mean=F3, std=F3, cmap=P, rows=256, a=256,
            outs=(P, P, None, None), code=P, scratch_bytes=1 << 30):
    from depthg_amd import _lib
    lib = _lib.load()
    rc = lib.dg_segment_labels(code, None, B, D, h, w, P, None, n, P, m, H, W, remap, img, mean, std, cmap, rows, a, *outs, P,
                               scratch_bytes, None)
    return rc, lib.dg_last_error().decode()


def _paint(G=2, B=2, H=8, W=8, m=4, img=None, cmap=P, rows=256, a=256, outs=(P, P, None, None), preds=P):
    from depthg_amd import _lib
    lib = _lib.load()
    rc = lib.dg_label_paint(preds, G, B, H, W, m, None, img, F3, F3, cmap, rows, a, *outs, None)
    return rc, lib.dg_last_error().decode()


def test_c_abi_refusals_come_before_any_launch():
    for kw in (dict(B=0), dict(D=0), dict(h=0), dict(w=0), dict(n=0), dict(m=0), dict(H=0), dict(W=0)):
        rc, msg = _labels(**kw)
        assert rc == -1 and "dimensions" in msg, (kw, rc, msg)
    rc, msg = _labels(n=256, m=1)
    assert rc == -2 and "n <= 255" in msg, msg
    rc, msg = _labels(n=1, m=256)
    assert rc == -2 and "m <= 255" in msg, msg
    rc, msg = _labels(n=200, m=57)
    assert rc == -2 and "n + m <= 256" in msg, msg
    rgb = (None, None, P, P)
    for rows in (0, -1, 257):
        rc, msg = _labels(outs=rgb, rows=rows)
        assert rc == -1 and "cmap_rows" in msg, (rows, msg)
    rc, msg = _labels(outs=rgb, cmap=None)
    assert rc == -1 and "cmap" in msg
    for a in (-1, 257):
        rc, msg = _labels(outs=rgb, a=a)
        assert rc == -1 and "alpha256" in msg, (a, msg)
    rc, msg = _labels(outs=rgb, a=255, img=None)
    assert rc == -1 and "img" in msg, msg
    rc, msg = _labels(outs=rgb, a=0, img=P, mean=None)
    assert rc == -1 and "mean" in msg, msg
    rc, msg = _labels(outs=(None,) * 4)
    assert rc == -1 and "nothing to write" in msg
    rc, msg = _labels(W=8177)
    assert rc == -2 and "W <= 8176" in msg, msg
    rc, msg = _labels(scratch_bytes=2 * 16 * 8 * 4 - 1)            # B*h*w*(4 + 4)*4 bytes needed
    assert rc == -3 and "scratch" in msg
    rc, msg = _labels(code=None)                                    # everything else in order: refused for the null pointer
    assert rc == -1 and "null" in msg
    # label outputs need neither a colour map nor an image, whatever alpha says
    rc, msg = _labels(cmap=None, rows=0, a=0, code=None)
    assert rc == -1 and "null" in msg, msg
    # dg_label_paint
    for kw in (dict(G=0), dict(B=0), dict(H=0), dict(W=0), dict(m=0)):
        rc, msg = _paint(**kw)
        assert rc == -1 and "dimensions" in msg, (kw, msg)
    rc, msg = _paint(m=256)
    assert rc == -2 and "m <= 255" in msg
    rc, msg = _paint(outs=rgb, rows=0)
    assert rc == -1 and "cmap_rows" in msg
    rc, msg = _paint(outs=rgb, a=128)
    assert rc == -1 and "img" in msg
    rc, msg = _paint(G=1)                                           # the cluster map is preds[1]
    assert rc == -1 and "preds[1]" in msg
    rc, msg = _paint(preds=None)
    assert rc == -1 and "null" in msg


def test_ops_refuse_bad_tables_and_cpu_tensors():
    from depthg_amd import ops
    code, lin_w, lin_b, clusters = torch.randn(2, 8, 4, 4), torch.randn(5, 8), torch.randn(5), torch.randn(7, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.segment_labels(code, lin_w, lin_b, clusters, 9, 9)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.label_paint(torch.zeros(2, 1, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="preds"):
        ops.label_paint(torch.zeros(2, 1, 4, 4, dtype=torch.int32))
    dev = torch.device("cpu")
    base = dict(dev=dev, B=2, H=4, W=4, m=7, remap=None, img=None, cmap=None, alpha=1.0, want=("lin",), mean=ops.IMAGENET_MEAN,
                std=ops.IMAGENET_STD, out=None)
    for over, match in ((dict(remap=[0, 1, 2, 3, 4, 5, 255]), "remap entries"), (dict(remap=[0, 1, 2, 3, 4, 5, -2]), "remap entries"),
                        (dict(remap=[0, 1, 2]), "remap must be"), (dict(remap=torch.zeros(7)), "remap must be"),
                        (dict(want=()), "want"), (dict(want=("lin", "depth")), "want"), (dict(alpha=1.5), "alpha"),
                        (dict(want=("lin_rgb",), alpha=0.5), "img is needed"),
                        (dict(want=("lin_rgb",), cmap=torch.zeros(300, 3, dtype=torch.uint8)), "cmap"),
                        (dict(out={"lin": torch.zeros(2, 4, 5, dtype=torch.uint8)}), "out")):
        with pytest.raises(ValueError, match=match):
            ops._paint_operands(**{**base, **over})


def test_default_colour_map_is_the_bit_interleave_rule():
    from depthg_amd import ops
    want = np.zeros((256, 3), np.uint8)
    for i in range(256):
        for bit in range(24):                       # bit `bit` of the id goes to channel bit % 3, at position 7 - bit // 3
            if bit // 3 < 8 and (i >> bit) & 1:
                want[i, bit % 3] |= 1 << (7 - bit // 3)
    got = ops.pascal_colormap()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (256, 3)
    assert np.array_equal(got.numpy(), want)
    # the well-known first rows of the PASCAL VOC palette
    assert got[:6].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128]]
    assert got[15].tolist() == [192, 128, 128] and got[255].tolist() == [224, 224, 192]
    assert torch.equal(ops.pascal_colormap(7), got[:7])


class _Metric:
    """An UnsupervisedMetrics stand-in with a given table."""

    def __init__(self, table):
        self.assignments = (np.arange(len(table)), np.asarray(table))
        self._table = torch.tensor(table)

    def map_clusters(self, clusters):
        return self._table[clusters]


def _probes(D, n, m, g):
    from depthg_amd.head import ClusterLookup
    linear, cluster = torch.nn.Conv2d(D, n, (1, 1)), ClusterLookup(D, m)
    with torch.no_grad():
        linear.weight.copy_(torch.randn(n, D, 1, 1, generator=g))
        linear.bias.copy_(torch.randn(n, generator=g) * 0.1)
        cluster.clusters.copy_(torch.randn(m, D, generator=g))
    return linear, cluster


def _normalised(B, H, W, g):
    from depthg_amd import ops
    raw = torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255
    mean, std = (torch.tensor(v).reshape(1, 3, 1, 1) for v in (ops.IMAGENET_MEAN, ops.IMAGENET_STD))
    return (raw - mean) / std, (raw * 255).round().to(torch.int64)


@pytest.mark.parametrize("flip", [False, True])
def test_cpu_route_is_the_reference_chain(flip):
    from depthg_amd import ops, segment
    from depthg_amd.evaluation import Segmentation
    g = torch.Generator().manual_seed(3)
    B, D, h, w, H, W, n, m = 2, 5, 3, 4, 7, 9, 3, 4
    code, code_flip = torch.randn(B, D, h, w, generator=g), torch.randn(B, D, h, w, generator=g) if flip else None
    linear, cluster = _probes(D, n, m, g)
    img, bytes_ = _normalised(B, H, W, g)
    table = [2, -1, 0, 1]
    # the reference's chain (src/demo_segmentation.py:59-78 without the CRF), written out
    with torch.no_grad():
        c = (code + code_flip.flip(dims=[3])) / 2 if flip else code
        up = F.interpolate(c, (H, W), mode="bilinear", align_corners=False)
        want_lin = linear(up).argmax(1)
        raw_clu = torch.einsum("bchw,nc->bnhw", F.normalize(up, dim=1), F.normalize(cluster.clusters, dim=1)).argmax(1)
    assert len(raw_clu.unique()) > 1 and (raw_clu == 1).any()                    # the -1 entry is used
    mapped = torch.tensor(table)[raw_clu]
    want_clu = torch.where(mapped < 0, torch.full_like(mapped, 255), mapped)
    cmap = ops.pascal_colormap().to(torch.int64)
    # raw cluster ids without a metric, as the reference demo stores them
    seg = segment(code, (H, W), linear, cluster, code_flip=code_flip)
    assert isinstance(seg, Segmentation) and seg.linear_rgb is None and seg.cluster_rgb is None
    assert seg.linear.dtype == torch.uint8 and tuple(seg.linear.shape) == (B, H, W)
    assert torch.equal(seg.linear.long(), want_lin) and torch.equal(seg.cluster.long(), raw_clu)
    for alpha in (0.0, 0.5, 1.0):
        seg = segment(code, (H, W), linear, cluster, code_flip=code_flip, cluster_metrics=_Metric(table),
                      img=None if alpha == 1.0 else img, overlay=alpha)
        assert torch.equal(seg.linear.long(), want_lin) and torch.equal(seg.cluster.long(), want_clu)
        a = int(round(alpha * 256))
        pix = bytes_.permute(0, 2, 3, 1)
        for got, lab in ((seg.linear_rgb, want_lin), (seg.cluster_rgb, want_clu)):
            assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, 3)
            want = (a * cmap[lab] + (256 - a) * pix + 128) >> 8
            assert torch.equal(got.long(), want), alpha
        if alpha == 0.0:
            assert torch.equal(seg.linear_rgb.long(), pix)                       # the image's own bytes come back
        if alpha == 1.0:
            assert torch.equal(seg.cluster_rgb.long(), cmap[want_clu])           # 255 paints the last row
    with pytest.raises(RuntimeError, match="GPU"):
        segment(code, (H, W), linear, cluster, run_crf=True, img=img)
    with pytest.raises(ValueError, match="img"):
        segment(code, (H, W), linear, cluster, overlay=0.5)
    with pytest.raises(ValueError, match="overlay"):
        segment(code, (H, W), linear, cluster, overlay=1.5)
    with pytest.raises(ValueError, match="size asked for"):
        segment(code, (H, W), linear, cluster, overlay=0.5, img=img[:, :, :5])


class _TinyNet(torch.nn.Module):
    """DinoFeaturizer's output contract on a strided convolution."""

    def __init__(self, dim, patch=8):
        super().__init__()
        self.patch_size, self.n_feats = patch, 12
        self.conv = torch.nn.Conv2d(3, dim, patch, stride=patch)

    def forward(self, img):
        code = self.conv(img)
        return (code, code, None) if self.training else (code, code)


def test_segmenter_segment_on_a_cpu_stand_in():
    from depthg_amd.evaluation import Segmentation
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(5)
    cfg = default_segmenter_cfg(dim=6, extra_clusters=2)
    model = UnsupervisedSegmenter(4, cfg, net=_TinyNet(6))
    model.train()
    img = torch.randn(3, 3, 16, 24)
    seg = model.segment(img)
    assert model.net.training                                                     # the mode it found
    assert isinstance(seg, Segmentation) and seg.linear_rgb is None
    for t in (seg.linear, seg.cluster):
        assert t.dtype == torch.uint8 and tuple(t.shape) == (3, 16, 24) and not t.requires_grad
    assert int(seg.linear.max()) < 4 and int(seg.cluster.max()) < 6              # raw ids: no assignment yet
    # flip=True is the average with the mirrored pass
    from depthg_amd import segment
    code, code_flip = model._eval_mode_codes(img, True)
    want = segment(code, (16, 24), model.linear_probe, model.cluster_probe, code_flip=code_flip)
    assert torch.equal(seg.linear, want.linear) and torch.equal(seg.cluster, want.cluster)
    # an assignment: test_cluster_metrics first, then cluster_metrics; remap=False keeps the raw ids
    model.cluster_metrics.stats = torch.randint(0, 50, (6, 4))
    model.cluster_metrics.compute()
    table = model.cluster_metrics.map_clusters(torch.arange(6))
    assert sorted(table.tolist()) == [-1, -1, 0, 1, 2, 3]
    seg2 = model.segment(img, overlay=0.25)
    mapped = table[seg.cluster.long()]
    assert torch.equal(seg2.cluster.long(), torch.where(mapped < 0, torch.full_like(mapped, 255), mapped))
    assert seg2.cluster_rgb.dtype == torch.uint8 and tuple(seg2.cluster_rgb.shape) == (3, 16, 24, 3)
    assert tuple(seg2.linear_rgb.shape) == (3, 16, 24, 3)
    assert torch.equal(model.segment(img, remap=False).cluster, seg.cluster)
    model.test_cluster_metrics.stats = torch.randint(0, 50, (6, 4))
    model.test_cluster_metrics.compute()
    table_t = model.test_cluster_metrics.map_clusters(torch.arange(6))
    mapped = table_t[seg.cluster.long()]
    assert torch.equal(model.segment(img).cluster.long(), torch.where(mapped < 0, torch.full_like(mapped, 255), mapped))
    with pytest.raises(ValueError, match="normalised images"):
        model.segment(img[0])


@pytest.mark.parametrize("overlay", [None, 0.5])
def test_demo_writes_the_label_images(tmp_path, overlay):
    from PIL import Image
    from depthg_amd import demo
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(9)
    rng = np.random.default_rng(9)
    images = tmp_path / "images"
    images.mkdir()
    for name, (hh, ww) in (("a.png", (20, 28)), ("b.one.png", (24, 16)), ("c.png", (16, 16))):
        Image.fromarray(rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8)).save(images / name)
    (images / "notes.txt").write_text("not an image")
    model = UnsupervisedSegmenter(4, default_segmenter_cfg(dim=6, extra_clusters=2))
    model.test_cluster_metrics.stats = torch.randint(0, 50, (6, 4))
    model.test_cluster_metrics.compute()
    ckpt = tmp_path / "model.pt"
    demo.save_checkpoint(model, str(ckpt))
    saved = torch.load(str(ckpt), map_location="cpu", weights_only=True)
    assert set(saved) == {"state_dict", "cfg", "n_classes", "cluster_assignments"} and saved["n_classes"] == 4
    assert saved["cfg"] == vars(model.cfg)
    out = tmp_path / "out"
    argv = ["--image-dir", str(images), "--out", str(out), "--checkpoint", str(ckpt), "--res", "16", "--batch-size", "2", "--cpu"]
    if overlay is not None:
        argv += ["--overlay", str(overlay)]
    assert demo.main(argv) == 0
    kinds = ["linear", "cluster"] + (["linear_rgb", "cluster_rgb"] if overlay is not None else [])
    assert sorted(os.listdir(out)) == sorted(kinds)
    names = ["a.png", "b.one.png", "c.png"]
    # what segment gives on the same images
    loaded = demo.load_checkpoint(str(ckpt))
    for k, v in model.state_dict().items():
        assert torch.equal(loaded.state_dict()[k], v), k
    assert not loaded.training
    loaded.net = demo.TorchHeadFeaturizer(loaded.net).eval()
    img = torch.stack([demo.load_image(str(images / n), 16) for n in names])
    assert tuple(img.shape) == (3, 3, 16, 16)
    want = loaded.segment(img, overlay=overlay)
    assert int((want.cluster == 255).sum()) > 0 or int(want.cluster.max()) < 4     # the assignment was applied
    for kind in kinds:
        assert sorted(os.listdir(out / kind)) == names
        for j, n in enumerate(names):
            with Image.open(out / kind / n) as im:
                assert im.mode == ("RGB" if kind.endswith("rgb") else "L") and im.size == (16, 16)
                assert np.array_equal(np.asarray(im), getattr(want, kind)[j].numpy()), (kind, n)
    with pytest.raises(FileNotFoundError, match="missing.pt"):
        demo.load_checkpoint(str(tmp_path / "missing.pt"))
    with pytest.raises(FileNotFoundError, match="nowhere"):
        demo.list_images(str(tmp_path / "nowhere"))


def test_load_image_resizes_the_shorter_side_and_crops_the_centre(tmp_path):
    from PIL import Image
    from depthg_amd import demo, ops
    arr = np.zeros((8, 16, 3), np.uint8)
    arr[:, :, 0] = np.arange(16, dtype=np.uint8)[None, :] * 10                   # red encodes the column
    Image.fromarray(arr).save(tmp_path / "wide.png")
    x = demo.load_image(str(tmp_path / "wide.png"), 8)
    assert tuple(x.shape) == (3, 8, 8) and x.dtype == torch.float32
    red = (x[0] * ops.IMAGENET_STD[0] + ops.IMAGENET_MEAN[0]) * 255
    assert torch.allclose(red[0], torch.arange(4, 12).float() * 10, atol=1e-3)    # columns 4..11: the centre crop
