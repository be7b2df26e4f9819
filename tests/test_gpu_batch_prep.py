"""dg_batch_prep (dg_batch.hip: k_batch_prep) against the plain chain of depthg_amd/data.py on the CPU - PIL's nearest resize and crop,
ToTensor, Normalize, ToTargetTensor (src/utils.py:164-182; src/data.py:87-132, 815-912): img bit for bit, label, mask and depth equal,
for samples of mixed sizes and their positives in ONE launch.  Every case runs with and without poisoned output buffers
(ops.POISON, the DG_POISON=1 hook): an element the kernel left out would be 0xFF bytes."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import data_folders as DF

pytestmark = pytest.mark.gpu

BIG = [(500, 375), (500, 375), (375, 500), (500, 375)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """The folders, written once: a cropped one with depth, a directory one with and one without labels, and the big sources."""
    root = tmp_path_factory.mktemp("data_path")
    out = {"cropped": str(root / "cropped"), "directory": str(root / "directory"), "bare": str(root / "bare"), "big": str(root / "big")}
    DF.make_cropped(out["cropped"])
    DF.make_directory(out["directory"])
    DF.make_directory(out["bare"], labels=False)
    DF.make_cropped(out["big"], sizes=BIG)
    for res in (16, 20):
        DF.write_nns(out["cropped"], "cocostuff27", "train", "five", res, len(DF.SIZES))
        DF.write_nns(out["directory"], "directory", "train", None, res, len(DF.SIZES))
        DF.write_nns(out["bare"], "directory", "train", None, res, len(DF.SIZES))
    DF.write_nns(out["big"], "cocostuff27", "train", "five", 224, len(BIG), k=3)
    return out


@pytest.fixture(params=[False, True], ids=["plain", "poison"])
def poison(request):
    from depthg_amd import ops
    old = ops.POISON
    ops.POISON = request.param or old
    yield
    ops.POISON = old


def _dataset(folders, kind, depth):
    from depthg_amd import data
    if kind == "cropped":
        return data.CroppedFolder(folders["cropped"], "cocostuff27", "five", 0.5, "train", return_depth=bool(depth),
                                  depth_type="zoedepth_plane" if depth == "plane" else "zoedepth")
    return data.DirectoryFolder(folders[kind], "train")


def _both_routes(ds, res, crop, inds, dev, cfg_res=None, seed=7):
    """The same batch from the CPU chain and from the kernel: same positives (global generator), same crop draws (`generator`)."""
    from depthg_amd import data
    cfg = SimpleNamespace(model_type=DF.MODEL_TYPE, res=cfg_res or res, num_neighbors=2)
    out = []
    for device in ("cpu", dev):
        batches = data.ContrastiveBatches(ds, cfg, "train", res, crop, len(inds), generator=torch.Generator().manual_seed(seed), num_workers=2,
                                          device=device)
        torch.manual_seed(seed)
        out.append(batches.batch_of(inds))
    return out


def _assert_same(want, got, dev):
    assert set(want) == set(got)
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), k
        if k in ("ind", "ind_pos"):
            assert torch.equal(g.cpu(), w)
            continue
        assert g.device == dev, k
        if w.dtype == torch.float32:          # bit for bit: -0.0 against 0.0 and a NaN would both show
            assert torch.equal(g.cpu().view(torch.int32), w.view(torch.int32)), (k, float((g.cpu() - w).abs().max()))
        else:
            assert torch.equal(g.cpu(), w), k


@pytest.mark.parametrize("res", [16, 20])
@pytest.mark.parametrize("crop", ["center", "random", None])
@pytest.mark.parametrize("kind,depth", [("cropped", True), ("cropped", False), ("cropped", "plane"), ("directory", False), ("bare", False)])
def test_batch_prep_matches_cpu_chain(kind, depth, crop, res, dev, folders, poison):
    """B = 3 samples plus 3 positives of five source sizes (wide, tall, square, 50 x 20, and 7 x 5 which is enlarged) in one launch;
    res 16 and 20: W is a multiple of 4 and not of the tile's 64 columns, H of 16 or not."""
    ds = _dataset(folders, kind, depth)
    want, got = _both_routes(ds, res, crop, [0, 3, 4], dev)
    sizes = {DF.SIZES[i] for i in want["ind"].tolist() + want["ind_pos"].tolist()}
    assert len(sizes) >= 4 and (7, 5) in sizes
    _assert_same(want, got, dev)
    assert ("depth" in got) == bool(depth)
    if depth == "plane":
        assert bool((got["depth"] == 255).all())
    # two calls give the same bytes
    again = _both_routes(ds, res, crop, [0, 3, 4], dev)[1]
    for k in got:
        assert torch.equal(got[k].cpu().view(torch.uint8) if got[k].dtype != torch.bool else got[k].cpu(),
                           again[k].cpu().view(torch.uint8) if again[k].dtype != torch.bool else again[k].cpu()), k


def test_batch_prep_at_the_loader_size(dev, folders, poison):
    """500 x 375 -> 224, B = 2 (+ 2 positives; one sample is 375 x 500): the size where the naive nearest rule leaves PIL's; 4 x 14 tiles."""
    from depthg_amd import data
    ds = data.CroppedFolder(folders["big"], "cocostuff27", "five", 0.5, "train", return_depth=True)
    want, got = _both_routes(ds, 224, "center", [1, 2], dev)
    assert tuple(got["img"].shape) == (2, 3, 224, 224) and tuple(got["depth_pos"].shape) == (2, 1, 224, 224)
    _assert_same(want, got, dev)


def _raw_call(dev, records, tables, H, W, packed_bytes=4096, img_offset=0, with_img=True):
    """dg_batch_prep itself on sentinel-filled outputs: (return code, message, outputs untouched)."""
    from depthg_amd import _lib
    lib = _lib.load()
    N = tables.shape[0]
    packed = torch.zeros(packed_bytes, dtype=torch.uint8, device=dev)
    img = torch.full((N * 3 * H * W + 4,), 7.0, device=dev)
    label = torch.full((N, H, W), 7, dtype=torch.int64, device=dev)
    mask = torch.full((N, H, W), 7.0, device=dev)
    depth = torch.full((N, H, W), 7.0, device=dev)
    params = torch.cat([records.reshape(-1), tables.reshape(-1)]).to(dev)
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    rc = lib.dg_batch_prep(packed.data_ptr(), packed.numel(), records.data_ptr(), tables.data_ptr(), params.data_ptr(), records.shape[0], N, H, W,
                           mean, std, img.data_ptr() + img_offset if with_img else None, label.data_ptr(), mask.data_ptr(), depth.data_ptr(),
                           torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    untouched = all(bool((t == 7).all()) for t in (img, label, mask, depth))
    return rc, lib.dg_last_error().decode(), untouched


def test_refusals_launch_nothing(dev):
    from depthg_amd import ops
    H = W = 16
    tables = torch.zeros((2, W + H), dtype=torch.int32)
    tables[:, :W] = torch.arange(W) % 8
    tables[:, W:] = torch.arange(H) % 6

    def recs(*rows):
        return torch.tensor(rows, dtype=torch.int32)

    image = lambda n, off=0, sw=8, sh=6: [ops.BATCH_IMAGE, n, off, 0, sw, sh, 0, 0]
    label = lambda n, rule=1, sw=8, sh=6: [ops.BATCH_LABEL, n, 300 + 48 * n, 0, sw, sh, 0, rule]
    plane = lambda n: [ops.BATCH_DEPTH_PLANE, n, 0, 0, 0, 0, 0, 0]
    good = recs(image(0), image(1, 144), label(0), label(1), plane(0), plane(1))
    rc, msg, untouched = _raw_call(dev, good, tables, H, W)
    assert rc == 0 and not untouched                                          # (the call the refusals below are one change away from)
    wide = tables.clone()
    wide[1, 3] = 8
    tall = tables.clone()
    tall[0, W + 2] = 6
    cases = [
        ("unknown kind", recs(image(0), [9, 1, 0, 0, 8, 6, 0, 0], label(0), label(1), plane(0), plane(1)), tables, {}),
        ("zero-sized source plane", recs(image(0), image(1, 144, sw=0), label(0), label(1), plane(0), plane(1)), tables, {}),
        ("narrower than the tables address", good, wide, {}),
        ("shorter than the tables address", good, tall, {}),
        ("leaves the packed buffer", recs(image(0), image(1, 4000), label(0), label(1), plane(0), plane(1)), tables, {}),
        ("16-byte aligned", good, tables, dict(img_offset=4)),
        ("written twice", recs(image(0), image(0, 144), label(0), label(1), plane(0), plane(1)), tables, {}),
        ("records for 1 of 2 samples", recs(image(0), image(1, 144), label(0), label(1), plane(0)), tables, {}),
        ("mask rule", recs(image(0), image(1, 144), label(0), label(1, rule=0), plane(0), plane(1)), tables, {}),
        ("output that is null", good, tables, dict(with_img=False)),
        ("above 16384 a side", recs(image(0, sw=20000, sh=1), image(1, 144), label(0), label(1), plane(0), plane(1)), tables, dict(packed_bytes=70000)),
    ]
    for text, records, tab, kw in cases:
        rc, msg, untouched = _raw_call(dev, records, tab, H, W, **kw)
        assert rc < 0 and text in msg and untouched, (text, rc, msg, untouched)
    # an output width that is no multiple of 4: no lane could store whole vectors
    odd = torch.zeros((2, 18 + 16), dtype=torch.int32)
    rc, msg, untouched = _raw_call(dev, good, odd, 16, 18)
    assert rc == -2 and "multiple of 4" in msg and untouched
    # and through the route: the library's message reaches the caller
    with pytest.raises(RuntimeError, match="unknown kind 9"):
        ops.batch_prep(torch.zeros(4096, dtype=torch.uint8), recs([9, 0, 0, 0, 8, 6, 0, 0]), tables[:1].contiguous(), (H, W), device=dev)
