"""`python -m depthg_amd.train` end to end on a folder of eight small images (src/train_segmentation.py:551-714 over
src/data.py:87-132): the nearest-neighbour table written first, three optimisation steps on batches the fused kernel prepared, the
validation, the checkpoints and the log."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import data_folders as DF
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [(120, 112), (112, 130), (128, 128), (150, 112), (112, 112), (140, 120), (113, 127), (131, 117)]


def test_train_command_three_steps(tmp_path):
    """The stand-in backbone at res 112 and dim 70 (the shapes of tests/test_segmenter.py's training step).  Four batches of two an
    epoch: val_freq = 2 exceeds a quarter of that and is dropped, as in the reference (:690-691), so the one validation is the one
    behind the fit's last step.  The command runs in a process of its own under a time limit; nothing in it may fault."""
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    DF.make_directory(root, sizes=SIZES, split="train", n_classes=5)
    DF.make_directory(root, sizes=SIZES[:4], split="val", n_classes=5, seed=2)
    args = ["--data-dir", root, "--out", out, "--dataset", "directory", "--precompute-knns", "res=112", "dim=70", "max_steps=3", "val_freq=2",
            "batch_size=2", "scalar_log_freq=1", "num_workers=2", "crop_type=~", "loader_crop_type=random", "num_neighbors=3",
            "use_depth=False", "depth_feat_correlation_loss=False", "depth_sampling=none", "dir_dataset_n_classes=5"]
    run = subprocess.run([sys.executable, "-m", "depthg_amd.train"] + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "3 step(s), 1 validation(s)" in run.stdout
    table = np.load(os.path.join(root, "nns", "nns_vit_small_directory_train_None_112.npz"))["nns"]
    assert table.shape == (8, 8) and table.dtype == np.int64                          # (eight images: eight columns)
    assert all(sorted(row.tolist()) == list(range(8)) for row in table)
    lines = [json.loads(l) for l in open(os.path.join(out, "log.jsonl"))]
    steps = [l for l in lines if "val" not in l]
    assert [l["step"] for l in steps] == [1, 2, 3]
    for l in steps:
        for key in ("loss/total", "loss/linear", "loss/cluster"):
            assert key in l and l[key] == l[key] and abs(l[key]) < float("inf"), (key, l)
    vals = [l for l in lines if "val" in l]
    assert len(vals) == 1 and vals[0]["step"] == 3 and "test/cluster/mIoU" in vals[0]["val"] and "test/linear/Accuracy" in vals[0]["val"]
    assert os.path.isfile(os.path.join(out, "best.pt"))

    from depthg_amd.demo import load_checkpoint
    model = load_checkpoint(os.path.join(out, "last.pt")).to("cuda:0")
    assert model.n_classes == 5 and model.cfg.res == 112
    seg = model.segment(torch.randn(2, 3, 112, 112, device="cuda:0"))
    assert tuple(seg.linear.shape) == (2, 112, 112) and tuple(seg.cluster.shape) == (2, 112, 112) and seg.linear.dtype == torch.uint8
    torch.cuda.synchronize()
