"""The training data path on the CPU (depthg_amd/data.py, depthg_amd/train.py): the index tables against PIL's own resize and crop,
the plain chain of ContrastiveBatches on folders written with PIL (src/data.py:87-132, 815-912, 1073-1141; src/utils.py:164-182), and
fit()'s schedule (src/train_segmentation.py:551-714) on a stub model that records its calls."""
import inspect
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import data_folders as DF

# (in_w, in_h, res): the small sizes with both crops, and the sizes where floor((d + 0.5) * in / out) leaves PIL's rule
TABLE_CASES = [(w, h, 16) for (w, h) in ((37, 23), (23, 37), (64, 64), (50, 20), (7, 5))] + [(500, 375, 224), (640, 427, 224), (1024, 2048, 224)]


def _pil_geometry(plane, res, crop_type, offsets=None):
    """Resize(res, NEAREST) and the cropper on one array, with PIL and torchvision's size rules spelled out once more."""
    h, w = plane.shape[:2]
    if crop_type is None:
        return np.asarray(Image.fromarray(plane).resize((res, res), Image.NEAREST))
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(res * long / short)
    nw, nh = (res, new_long) if w <= h else (new_long, res)
    im = Image.fromarray(plane).resize((nw, nh), Image.NEAREST)
    top, left = (int(round((nh - res) / 2.0)), int(round((nw - res) / 2.0))) if crop_type == "center" else offsets
    return np.asarray(im.crop((left, top, left + res, top + res)))


@pytest.mark.parametrize("crop_type", ["center", None])
@pytest.mark.parametrize("in_w,in_h,res", TABLE_CASES)
def test_index_tables_match_pil_resize_and_crop(in_w, in_h, res, crop_type):
    """Every pixel of the source carries its own index (mode "I"), so a wrong source row or column shows wherever it falls."""
    from depthg_amd.data import loader_index_tables
    src = np.arange(in_w * in_h, dtype=np.int32).reshape(in_h, in_w)
    want = _pil_geometry(src, res, crop_type)
    xs, ys, out_size = loader_index_tables(in_w, in_h, res, crop_type)
    assert out_size == (res, res) and xs.dtype == np.int32 and ys.dtype == np.int32 and xs.shape == (res,) and ys.shape == (res,)
    assert np.array_equal(src[np.ix_(ys, xs)], want)


def test_index_tables_random_crop_and_refusals():
    from depthg_amd import data
    src = np.arange(50 * 20, dtype=np.int32).reshape(20, 50)
    nw, nh = data.resized_size(50, 20, 16, "random")
    assert (nw, nh) == (40, 16)
    for left in (0, 7, 24):
        xs, ys, _ = data.loader_index_tables(50, 20, 16, "random", offsets=(0, left))
        assert np.array_equal(src[np.ix_(ys, xs)], _pil_geometry(src, 16, "random", (0, left)))
    # the offsets are RandomCrop's draws: the row offset first, then the column offset, none when the size already fits
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    top, left = data.draw_random_crop(40, 18, 16, g1)
    assert top == int(torch.randint(0, 3, (1,), generator=g2)) and left == int(torch.randint(0, 25, (1,), generator=g2))
    assert data.draw_random_crop(16, 16, 16, g1) == (0, 0) and torch.equal(g1.get_state(), g2.get_state())
    with pytest.raises(ValueError, match="offsets"):
        data.loader_index_tables(50, 20, 16, "random")
    with pytest.raises(ValueError, match="leave the resized image"):
        data.loader_index_tables(50, 20, 16, "random", offsets=(0, 25))
    with pytest.raises(ValueError, match="Unknown Cropper"):
        data.loader_index_tables(50, 20, 16, "five")
    with pytest.raises(ValueError, match="CenterCrop would pad"):
        data.center_crop_offset(15, 16)
    assert data.center_crop_offset(21, 16) == 2 and data.center_crop_offset(19, 16) == 2 and data.center_crop_offset(17, 16) == 0     # round half to even


def test_exports_and_signatures():
    import depthg_amd
    from depthg_amd import _lib, data, ops, train
    for name in ("ContrastiveBatches", "CroppedFolder", "DirectoryFolder", "loader_index_tables", "precompute_knns"):
        assert getattr(depthg_amd, name) is getattr(data, name) and name in depthg_amd.__all__
    assert "dg_batch_prep" in _lib.SIGNATURES and hasattr(_lib.load(), "dg_batch_prep") and callable(ops.batch_prep)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "depthg_corr.h")).read()
    assert "int dg_batch_prep(" in header
    assert list(inspect.signature(data.loader_index_tables).parameters) == ["in_w", "in_h", "res", "crop_type", "offsets"]
    assert list(inspect.signature(data.ContrastiveBatches.__init__).parameters)[1:12] == [
        "dataset", "cfg", "image_set", "res", "loader_crop_type", "batch_size", "shuffle", "generator", "num_workers", "pos", "return_depth"]
    assert list(inspect.signature(data.precompute_knns).parameters)[:6] == ["net", "dataset", "cfg", "res", "image_set", "crop_type"]
    assert list(inspect.signature(train.fit).parameters)[:5] == ["model", "train_batches", "val_batches", "cfg", "out_dir"]
    assert data.MAX_DECODE_THREADS == 16


def _cfg(res, num_neighbors=3):
    return SimpleNamespace(model_type=DF.MODEL_TYPE, res=res, num_neighbors=num_neighbors)


def test_cropped_folder_cpu_route(tmp_path):
    """CroppedDataset's contract after default collation: label = byte - 1 (B,H,W), mask = (label == -1) bool (B,1,H,W), depth the
    byte as float (B,1,H,W), the positive's planes beside them - against the folder's own files through PIL."""
    from depthg_amd import data
    root, res, B = str(tmp_path), 16, 3
    DF.make_cropped(root)
    table = DF.write_nns(root, "cocostuff27", "train", "five", res, len(DF.SIZES))
    ds = data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train", return_depth=True)
    assert len(ds) == len(DF.SIZES) and ds.n_classes == 27
    batches = data.ContrastiveBatches(ds, _cfg(res), "train", res, "center", B, shuffle=False, generator=None, num_workers=2, device="cpu")
    assert len(batches) == 3
    torch.manual_seed(0)
    got = list(batches)
    assert [len(b["ind"]) for b in got] == [3, 3, 2]
    batch = got[0]
    assert set(batch) == {"ind", "img", "label", "mask", "depth", "img_pos", "ind_pos", "depth_pos", "label_pos", "mask_pos"}
    want = {"ind": ((B,), torch.int64), "ind_pos": ((B,), torch.int64), "img": ((B, 3, res, res), torch.float32),
            "img_pos": ((B, 3, res, res), torch.float32), "label": ((B, res, res), torch.int64), "label_pos": ((B, res, res), torch.int64),
            "mask": ((B, 1, res, res), torch.bool), "mask_pos": ((B, 1, res, res), torch.bool),
            "depth": ((B, 1, res, res), torch.float32), "depth_pos": ((B, 1, res, res), torch.float32)}
    for k, (shape, dtype) in want.items():
        assert tuple(batch[k].shape) == shape and batch[k].dtype == dtype, k
    assert batch["ind"].tolist() == [0, 1, 2]
    mean, std = (torch.tensor(v, dtype=torch.float32).reshape(3, 1, 1) for v in ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
    base = os.path.join(root, "cropped", "cocostuff27_five_crop_0.5")
    for b in got:
        for j, (i, ip) in enumerate(zip(b["ind"].tolist(), b["ind_pos"].tolist())):
            assert ip in table[i][1:4] and ip != i                       # columns 1 .. num_neighbors of the table
            for idx, suffix in ((i, ""), (ip, "_pos")):
                img = np.asarray(Image.open(os.path.join(base, "img", "train", f"{idx}.jpg")).convert("RGB"))
                x = torch.from_numpy(_pil_geometry(img, res, "center").copy()).permute(2, 0, 1).float().div(255)
                assert torch.equal(b["img" + suffix][j], (x - mean) / std)
                lab = _pil_geometry(np.asarray(Image.open(os.path.join(base, "label", "train", f"{idx}.png"))), res, "center").astype(np.int64) - 1
                assert np.array_equal(b["label" + suffix][j].numpy(), lab)
                assert np.array_equal(b["mask" + suffix][j, 0].numpy(), lab == -1)
                dep = _pil_geometry(np.asarray(Image.open(os.path.join(base, "depth", "train", f"{idx}_zoedepth.png"))), res, "center")
                assert np.array_equal(b["depth" + suffix][j, 0].numpy(), dep.astype(np.float32))
    assert any((b["label"] == -1).any() for b in got) and any((b["label"] == 26).any() for b in got)
    # the positive is drawn, not fixed: every one of the columns 1 .. 3 turns up
    seen = set()
    for _ in range(6):
        for b in batches:
            seen.update((int(ip) - int(i)) % len(DF.SIZES) for i, ip in zip(b["ind"], b["ind_pos"]))
    assert seen == {1, 2, 3}
    # no depth asked: the keys are absent; the plane variant: a constant 255 map and no depth file is read
    nodepth = data.ContrastiveBatches(ds, _cfg(res), "train", res, "center", B, num_workers=0, return_depth=False, device="cpu").batch_of([0, 4])
    assert "depth" not in nodepth and "depth_pos" not in nodepth
    plane = data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train", return_depth=True, depth_type="zoedepth_plane")
    assert plane.plane_depth and plane.depth_type == "zoedepth" and plane.root == ds.root
    pb = data.ContrastiveBatches(plane, _cfg(res), "train", res, None, B, device="cpu").batch_of([3, 4])
    assert torch.equal(pb["depth"], torch.full((2, 1, res, res), 255.0)) and torch.equal(pb["depth_pos"], torch.full((2, 1, res, res), 255.0))
    # shuffling follows the generator
    order = [b["ind"].tolist() for b in data.ContrastiveBatches(ds, _cfg(res), "train", res, "center", B, shuffle=True,
                                                                generator=torch.Generator().manual_seed(3), device="cpu")]
    assert sum(order, []) == torch.randperm(len(DF.SIZES), generator=torch.Generator().manual_seed(3)).tolist()


def test_directory_folder_cpu_route(tmp_path):
    """DirectoryDataset's contract: files paired by sorted position, the label as stored (B,1,H,W), mask = (label > 0) float32
    (B,1,H,W); without a labels folder label -1 and mask 0, both (B,H,W)."""
    from depthg_amd import data
    root, res = str(tmp_path / "with"), 16
    written = DF.make_directory(root)
    DF.write_nns(root, "mine", "train", None, res, len(DF.SIZES))
    ds = data.DirectoryFolder(root, "train", name="mine", n_classes=5)
    batches = data.ContrastiveBatches(ds, _cfg(res), "train", res, None, 4, device="cpu")
    torch.manual_seed(1)
    b = batches.batch_of([4, 0, 3, 6])
    assert set(b) == {"ind", "img", "label", "mask", "img_pos", "ind_pos", "label_pos", "mask_pos"}
    assert tuple(b["label"].shape) == (4, 1, res, res) and b["label"].dtype == torch.int64
    assert tuple(b["mask"].shape) == (4, 1, res, res) and b["mask"].dtype == torch.float32
    mean, std = (torch.tensor(v, dtype=torch.float32).reshape(3, 1, 1) for v in ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
    for j, (i, ip) in enumerate(zip(b["ind"].tolist(), b["ind_pos"].tolist())):
        for idx, suffix in ((i, ""), (ip, "_pos")):
            image, label, _ = written[idx]
            x = torch.from_numpy(_pil_geometry(image, res, None).copy()).permute(2, 0, 1).float().div(255)
            assert torch.equal(b["img" + suffix][j], (x - mean) / std)
            lab = _pil_geometry(label, res, None).astype(np.int64)
            assert np.array_equal(b["label" + suffix][j, 0].numpy(), lab)
            assert np.array_equal(b["mask" + suffix][j, 0].numpy(), (lab > 0).astype(np.float32))
    assert (b["label"] == 0).any() and (b["mask"] == 0).any() and (b["mask"] == 1).any()
    # no labels folder
    bare = str(tmp_path / "bare")
    DF.make_directory(bare, labels=False)
    ds2 = data.DirectoryFolder(bare, "train")
    nb = data.ContrastiveBatches(ds2, _cfg(res), "train", res, "center", 2, pos=False, device="cpu").batch_of([1, 2])
    assert set(nb) == {"ind", "img", "label", "mask"}
    assert torch.equal(nb["label"], torch.full((2, res, res), -1, dtype=torch.int64)) and torch.equal(nb["mask"], torch.zeros(2, res, res))


def test_missing_table_and_16_bit_label_are_refused(tmp_path):
    from depthg_amd import data
    root, res = str(tmp_path), 16
    DF.make_cropped(root)
    ds = data.CroppedFolder(root, "cocostuff27", "five", 0.5, "train")
    with pytest.raises(ValueError, match="could not find nn file .*nns_vit_small_cocostuff27_train_five_16.npz please run precompute_knns"):
        data.ContrastiveBatches(ds, _cfg(res), "train", res, "center", 2, device="cpu")
    path = os.path.join(ds.label_dir, "2.png")
    Image.fromarray(np.full((64, 64), 300, dtype=np.uint16)).save(path)
    with pytest.raises(ValueError, match=r"label .*2\.png.* has PIL mode 'I;16'"):
        data.ContrastiveBatches(ds, _cfg(res), "train", res, "center", 2, pos=False, device="cpu").batch_of([2])
    with pytest.raises(FileNotFoundError, match="no image folder"):
        data.CroppedFolder(root, "cocostuff27", "five", 0.5, "test")
    # nyuv2 and the non-zoedepth depth types keep the depth type in the folder's name (src/data.py:825-833)
    for name, depth_type, want in (("nyuv2", "zoedepth", "nyuv2_five_crop_0.5_zoedepth"), ("potsdam", "gt", "potsdam_five_crop_0.5_gt")):
        with pytest.raises(FileNotFoundError, match=want):
            data.CroppedFolder(root, name, "five", 0.5, "train", depth_type=depth_type)


class _StubModel:
    """training_step / validation_step / on_validation_epoch_end that record their calls; the monitored metric follows `scores`."""

    def __init__(self, scores):
        self.calls, self.scores, self.step = [], list(scores), 0

    def training_step(self, batch, batch_idx):
        self.step += 1
        self.calls.append(("train", batch, batch_idx))
        return torch.tensor(float(self.step)), {"loss/total": torch.tensor(float(self.step)), "hist/x": torch.tensor([1, 2])}

    def validation_step(self, batch, batch_idx):
        self.calls.append(("val", batch, batch_idx))

    def on_validation_epoch_end(self):
        self.calls.append(("val_end", self.step, None))
        s = self.scores.pop(0)
        return {"test/cluster/mIoU": s, "test/cluster/Accuracy": 100.0 - s}


def _run_fit(tmp_path, name, n_batches, scores, **cfg_kw):
    from depthg_amd import train
    saved = []
    model = _StubModel(scores)
    cfg = SimpleNamespace(**{**dict(max_steps=10, val_freq=2, scalar_log_freq=3, dataset_name="cocostuff27"), **cfg_kw})
    out = str(tmp_path / name)
    state = train.fit(model, list(range(n_batches)), ["a", "b"], cfg, out, save_checkpoint=lambda m, p: saved.append((os.path.basename(p), m.step)))
    lines = [json.loads(l) for l in open(os.path.join(out, "log.jsonl"))]
    return model, state, saved, lines


def test_fit_schedule_on_a_stub_model(tmp_path):
    # 8 batches an epoch, val_freq 2 <= 8 // 4: validation behind every second batch of an epoch; max_steps 10 ends in the second epoch
    model, state, saved, lines = _run_fit(tmp_path, "a", 8, [1.0, 5.0, 3.0, 5.0, 7.0])
    assert state["steps"] == 10 and state["val_steps"] == [2, 4, 6, 8, 10] and state["validations"] == 5
    assert [(c[1], c[2]) for c in model.calls if c[0] == "train"] == [(i % 8, i % 8) for i in range(10)]
    assert [c[1:] for c in model.calls if c[0] == "val"] == [("a", 0), ("b", 1)] * 5
    # best.pt only when the monitored metric EXCEEDS its best (5.0 twice: one save); last.pt behind every validation and at the end
    assert [s for s in saved if s[0] == "best.pt"] == [("best.pt", 2), ("best.pt", 4), ("best.pt", 10)]
    assert [s[1] for s in saved if s[0] == "last.pt"] == [2, 4, 6, 8, 10, 10]
    assert state["best"] == 7.0 and state["best_step"] == 10 and state["losses"] == [float(i) for i in range(1, 11)]
    # the step's logs every scalar_log_freq steps, tensors as numbers and lists; one line per validation
    assert [l["step"] for l in lines if "val" not in l] == [3, 6, 9]
    assert lines[0] == {"step": 2, "val": {"test/cluster/mIoU": 1.0, "test/cluster/Accuracy": 99.0}}
    assert next(l for l in lines if l["step"] == 3) == {"step": 3, "loss/total": 3.0, "hist/x": [1, 2]}

    # val_freq above a quarter of an epoch is dropped: validation at the end of every epoch, and behind the fit's last step
    model, state, saved, _ = _run_fit(tmp_path, "b", 4, [2.0, 1.0, 0.5], val_freq=2)
    assert state["val_steps"] == [4, 8, 10] and [s for s in saved if s[0] == "best.pt"] == [("best.pt", 4)]
    # ... so a fit shorter than an epoch validates once, behind its last step
    model, state, saved, _ = _run_fit(tmp_path, "c", 4, [2.0], max_steps=3)
    assert state["steps"] == 3 and state["val_steps"] == [3] and saved == [("last.pt", 3), ("best.pt", 3), ("last.pt", 3)]
    # potsdam monitors the accuracy
    model, state, saved, _ = _run_fit(tmp_path, "d", 8, [1.0, 5.0], max_steps=4, dataset_name="potsdam")
    assert state["best"] == 99.0 and state["best_step"] == 2


def test_train_cfg_and_overrides():
    from depthg_amd import train
    over = train.parse_overrides(["res=112", "crop_type=~", "dataset_name=directory", "lr=1e-3", "use_depth=False", "dir_dataset_name=mine"])
    assert over == {"res": 112, "crop_type": None, "dataset_name": "directory", "lr": 1e-3, "use_depth": False, "dir_dataset_name": "mine"}
    cfg = train.build_cfg(over)
    assert cfg.res == 112 and cfg.batch_size == 32 and cfg.val_freq == 100 and cfg.dim == 70 and cfg.num_neighbors == 7
    with pytest.raises(ValueError, match="Unexpected arg style"):
        train.parse_overrides(["--res"])
    assert train.validation_interval(cfg, 400) == 100 and train.validation_interval(cfg, 399) is None
