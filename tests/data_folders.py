"""Dataset folders for the data-path tests (tests/test_data_cpu.py, test_gpu_batch_prep.py, test_gpu_train_loop.py): small images
written with PIL in the layouts of the reference's CroppedDataset (src/data.py:815-912) and DirectoryDataset (src/data.py:87-132), and
a nearest-neighbour table in the reference's file format (src/precompute_knns.py:115)."""
import os

import numpy as np
from PIL import Image

# (width, height): wide, tall, square, a side that is no multiple of anything, and one the loader has to enlarge
SIZES = [(37, 23), (23, 37), (64, 64), (50, 20), (7, 5), (64, 64), (23, 37), (37, 23)]
MODEL_TYPE = "vit_small"


def _planes(rng, w, h, n_label):
    image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    label = rng.integers(0, n_label, (h, w), dtype=np.uint8)
    depth = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return image, label, depth


def make_cropped(root, sizes=SIZES, split="train", name="cocostuff27", crop="five", ratio=0.5, depth_type="zoedepth", seed=0):
    """<root>/cropped/{name}_{crop}_crop_{ratio}/{img,label,depth}/{split}/: {i}.jpg, {i}.png (bytes 0 .. 27: label -1 .. 26 behind the
    dataset's offset), {i}_{depth_type}.png.  Returns the planes as written, [(image, label, depth)] (the image before JPEG coding)."""
    rng = np.random.default_rng(seed)
    base = os.path.join(root, "cropped", "{}_{}_crop_{}".format(name, crop, ratio))
    for kind in ("img", "label", "depth"):
        os.makedirs(os.path.join(base, kind, split), exist_ok=True)
    out = []
    for i, (w, h) in enumerate(sizes):
        image, label, depth = _planes(rng, w, h, 28)
        Image.fromarray(image).save(os.path.join(base, "img", split, f"{i}.jpg"), quality=95)
        Image.fromarray(label).save(os.path.join(base, "label", split, f"{i}.png"))
        Image.fromarray(depth).save(os.path.join(base, "depth", split, f"{i}_{depth_type}.png"))
        out.append((image, label, depth))
    return out


def make_directory(root, sizes=SIZES, split="train", labels=True, n_classes=5, seed=1):
    """<root>/imgs/{split}/img_{i:03d}.png and <root>/labels/{split}/img_{i:03d}.png (bytes 0 .. n_classes - 1).  PNG: the planes
    returned are the planes a reader decodes."""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "imgs", split), exist_ok=True)
    if labels:
        os.makedirs(os.path.join(root, "labels", split), exist_ok=True)
    out = []
    for i, (w, h) in enumerate(sizes):
        image, label, _ = _planes(rng, w, h, n_classes)
        Image.fromarray(image).save(os.path.join(root, "imgs", split, f"img_{i:03d}.png"))
        if labels:
            Image.fromarray(label).save(os.path.join(root, "labels", split, f"img_{i:03d}.png"))
        out.append((image, label if labels else None, None))
    return out


def write_nns(root, name, split, crop, res, n, k=4, model_type=MODEL_TYPE):
    """nns/nns_{model}_{name}_{split}_{crop}_{res}.npz: row i = [i, i + 1, ..., i + k - 1] mod n.  Returns the table."""
    table = (np.arange(n)[:, None] + np.arange(k)[None, :]) % n
    os.makedirs(os.path.join(root, "nns"), exist_ok=True)
    np.savez_compressed(os.path.join(root, "nns", "nns_{}_{}_{}_{}_{}.npz".format(model_type, name, split, crop, res)), nns=table.astype(np.int64))
    return table
