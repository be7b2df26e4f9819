"""Inputs of the sample-cache tests (tests/test_sample_cache_cpu.py, tests/test_gpu_sample_cache.py): in-memory datasets of decoded
samples whose planes carry the extreme bytes, and a bitwise comparison."""
import numpy as np
import torch

from depthg_amd import data, ops


class MemorySet:
    """What the data path reads of a dataset - load, __len__, has_labels, label_offset, mask_rule, label_dims, return_depth - over
    samples held in memory; `loads` counts the calls of `load`."""

    def __init__(self, samples, label_offset, mask_rule):
        self.samples, self.label_offset, self.mask_rule = samples, label_offset, mask_rule
        self.has_labels = samples[0].label is not None
        self.return_depth = samples[0].depth is not None
        self.label_dims, self.nns_name, self.crop_type, self.split, self.loads = 3, "memory", None, "train", 0

    def __len__(self):
        return len(self.samples)

    def load(self, index):
        self.loads += 1
        return self.samples[int(index)]


def make_samples(sizes, labels=True, depth="bytes", n_label=28, seed=0):
    """data.Sample per (width, height): random planes with the bytes 0 and 255 written into every plane's corners and centre (a nearest
    resize keeps some of them at every size used here).  depth: "bytes", "plane" (data.PLANE) or None."""
    rng = np.random.default_rng(seed)
    out = []
    for w, h in sizes:
        image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        label = rng.integers(0, n_label, (h, w), dtype=np.uint8) if labels else None
        d = rng.integers(0, 256, (h, w), dtype=np.uint8) if depth == "bytes" else (data.PLANE if depth == "plane" else None)
        for plane in (image, label, d):
            if isinstance(plane, np.ndarray):
                plane[:h // 2, :w // 2] = np.where(rng.random((h // 2, w // 2) + plane.shape[2:]) < 0.25, 0, plane[:h // 2, :w // 2])
                plane[h // 2:, w // 2:] = np.where(rng.random((h - h // 2, w - w // 2) + plane.shape[2:]) < 0.25, 255, plane[h // 2:, w // 2:])
        out.append(data.Sample(image, label, d))
    return out


def chain(dataset, samples, res, crop_type, want_depth):
    """data._cpu_chain of every sample, stacked: (img, label, mask, depth or None)."""
    rows = [data._cpu_chain(dataset, s, res, crop_type, None, want_depth) for s in samples]
    img, label, mask = (torch.stack([r[k] for r in rows]) for k in range(3))
    return img, label, mask, (torch.stack([r[3] for r in rows]) if want_depth else None)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


CROPPED = dict(label_offset=-1, mask_rule=ops.BATCH_MASK_BOOL_IGNORED)        # CroppedFolder's rules
DIRECTORY = dict(label_offset=0, mask_rule=ops.BATCH_MASK_FLOAT_POSITIVE)     # DirectoryFolder's
