"""The training data path: folder datasets, the loader transform of a whole batch as one fused HIP launch, the batch iterable
`training_step` reads, and the offline nearest-neighbour table.

The reference's loader (src/data.py:1073-1141 over src/data.py:87-132 / 815-912 and src/utils.py:164-182) runs, per sample and in CPU
workers, `Resize(res, NEAREST) -> cropper -> ToTensor -> Normalize` on the image and `Resize(res, NEAREST) -> cropper ->
ToTargetTensor` on the label and the depth map - four to six times per training sample (image, label, depth of the sample and of its
kNN positive).  All of it is a gather per output pixel and two float32 operations, so here only the decoding stays on the CPU:

    CroppedFolder / DirectoryFolder   the folder layouts of CroppedDataset / DirectoryDataset; `load(i)` returns the decoded uint8
                                      arrays at source size, no transform
    loader_index_tables               resize and crop composed into one source column per output column and one source row per
                                      output row; the per-axis indices of the resize come from PIL itself (a resized index ramp)
    pack_batch                        the decoded planes of 2B samples in one pinned byte buffer, one record per output plane group,
                                      the two index tables per sample
    ops.batch_prep                    one upload of the bytes, one of the tables, ONE launch (dg_batch_prep, dg_batch.hip) that
                                      writes img / label / mask / depth of the samples and the positives
    ContrastiveBatches                the iterable: shuffling, the kNN positive (knn.load_nns / knn.pick_positive), decoding in a small
                                      thread pool, and the dictionary of default collation - ind, img, label, mask, depth, img_pos,
                                      ind_pos, depth_pos, label_pos, mask_pos.  On a CPU device the same class runs the plain chain
                                      (PIL resize, crop, the torch operations): the restatement the GPU route is tested against.
    precompute_knns                   src/precompute_knns.py:15-21, 85-115 on centre-cropped batches through the same kernel
    build_feature_cache               one pass of the frozen backbone over a split with a deterministic loader transform, kept as a
                                      feature_cache.FeatureCache; ContrastiveBatches(feature_cache=...) then adds `image_feat` /
                                      `image_feat_pos` to every batch (cfg.dg_feature_cache in the step)
    build_sample_cache                one decoding pass over a split with a deterministic loader transform, kept as the transform's
                                      output BYTES in a sample_cache.SampleCache on the device; ContrastiveBatches(sample_cache=...)
                                      then forms img / label / mask / depth of a batch and its positives with one launch from the
                                      indices alone: a cached epoch opens no file

`img_aug` / `coord_aug` are not made here: cfg.dg_gpu_augment forms them inside the step (depthg_amd/augment.py).
"""
import functools
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

from . import knn, ops

MAX_DECODE_THREADS = 16       # the decoding pool never grows past this, whatever num_workers says and however many CPUs the host shows


def _decode_threads(num_workers):
    return max(0, min(int(num_workers), MAX_DECODE_THREADS))


def _default_device(device):
    """`device`, or without one the first GPU if there is one, else the CPU."""
    return ("cuda:0" if torch.cuda.is_available() else "cpu") if device is None else device


def _refuse_random_crop(crop_type, subject, what):
    """A cache keeps ONE view of every image: `subject` (the message's opening, its prefix included) refuses the random cropper."""
    if crop_type == "random":
        raise ValueError(f"{subject} with loader_crop_type = 'random': the {what} of an image would depend on the crop's draw; use 'center' or None")

# decoded planes of one sample: image (h, w, 3) uint8; label (h, w) uint8 or None; depth (h, w) uint8, None, or PLANE
Sample = namedtuple("Sample", "image label depth")
PLANE = "plane"               # Sample.depth of the `_plane` depth types: a constant 255 map, no file is read (src/data.py:897-898)

N_CLASSES = {"cityscapes": 27, "cocostuff27": 27, "nyuv2": 14, "pascalvoc": 21, "potsdam": 3}      # src/data.py:962-1037


# --------------------------------------------------------------------------------------------------------------- index tables
@functools.lru_cache(maxsize=None)
def _pil_nearest_axis(n_in, n_out, axis):
    """The source index PIL's `resize(..., NEAREST)` reads for each of the n_out outputs of an axis of n_in pixels - taken from PIL:
    a ramp 0 .. n_in - 1 (mode "I") along that axis, resized.  (PIL steps its source coordinate by additions in double; neither
    floor((d + 0.5) * n_in / n_out) nor floor(d * s + s / 2) reproduces that at sizes like 500 -> 298.)"""
    from PIL import Image
    ramp = np.arange(n_in, dtype=np.int32)
    if axis == 0:          # columns
        out = Image.fromarray(ramp.reshape(1, n_in)).resize((n_out, 1), Image.NEAREST)
    else:                  # rows
        out = Image.fromarray(ramp.reshape(n_in, 1)).resize((1, n_out), Image.NEAREST)
    idx = np.asarray(out, dtype=np.int32).reshape(-1).copy()
    assert idx.shape == (n_out,) and idx.min() >= 0 and idx.max() < n_in
    idx.setflags(write=False)
    return idx


def resized_size(in_w, in_h, res, crop_type):
    """(width, height) behind the transform's Resize (src/utils.py:164-182): `Resize((res, res))` when crop_type is None, else
    torchvision's `Resize(res)` - the shorter side to res, the other to int(res * long / short)."""
    in_w, in_h, res = int(in_w), int(in_h), int(res)
    if in_w < 1 or in_h < 1 or res < 1:
        raise ValueError(f"depthg_amd.data: image {in_w}x{in_h} and res {res} must be positive")
    if crop_type is None:
        return res, res
    if crop_type not in ("center", "random"):
        raise ValueError("Unknown Cropper {}".format(crop_type))                # src/utils.py:173
    short, long = (in_w, in_h) if in_w <= in_h else (in_h, in_w)
    new_long = int(res * long / short)
    return (res, new_long) if in_w <= in_h else (new_long, res)


def draw_random_crop(new_w, new_h, res, generator=None):
    """RandomCrop(res)'s (top, left) on an image of new_w x new_h: no draw when the image already has the size, else the row offset
    and then the column offset from torch's CPU generator, each `randint(0, side - res + 1)`."""
    if new_w < res or new_h < res:
        raise ValueError(f"depthg_amd.data: a random crop of {res} does not fit the resized image {new_w}x{new_h}")
    if new_w == res and new_h == res:
        return 0, 0
    top = int(torch.randint(0, new_h - res + 1, size=(1,), generator=generator).item())
    left = int(torch.randint(0, new_w - res + 1, size=(1,), generator=generator).item())
    return top, left


def center_crop_offset(size, res):
    """CenterCrop(res)'s offset on a side of `size` pixels, int(round((size - res) / 2.0)); a side below res - where CenterCrop pads
    with zeros first - is refused."""
    if size < res:
        raise ValueError(f"depthg_amd.data: a side of {size} pixels is smaller than the centre crop of {res}: CenterCrop would pad it with "
                         "zeros, which this loader does not do")
    return int(round((size - res) / 2.0))


def loader_index_tables(in_w, in_h, res, crop_type, offsets=None):
    """(xs, ys, (out_h, out_w)): int32 source column per output column and source row per output row of the loader transform on
    an image of in_w x in_h - nearest-neighbour resize (PIL's rule), then the crop: None (no crop: the resize is to res x res),
    "center" (CenterCrop's offset int(round((size - res) / 2.0)); its padding case - a resized side below res - is refused) or
    "random" with `offsets` = (top, left) drawn by the caller (draw_random_crop)."""
    res = int(res)
    new_w, new_h = resized_size(in_w, in_h, res, crop_type)
    col, row = _pil_nearest_axis(int(in_w), new_w, 0), _pil_nearest_axis(int(in_h), new_h, 1)
    if crop_type is None:
        if offsets is not None:
            raise ValueError("depthg_amd.data: crop offsets were given but crop_type is None")
        return col, row, (res, res)
    if crop_type == "center":
        if offsets is not None:
            raise ValueError("depthg_amd.data: crop offsets were given but crop_type is 'center'")
        top, left = center_crop_offset(new_h, res), center_crop_offset(new_w, res)
    else:
        if offsets is None:
            raise ValueError("depthg_amd.data: crop_type 'random' needs offsets=(top, left) (draw_random_crop draws them)")
        top, left = int(offsets[0]), int(offsets[1])
        if not (0 <= top <= new_h - res and 0 <= left <= new_w - res):
            raise ValueError(f"depthg_amd.data: crop offsets {(top, left)} leave the resized image {new_w}x{new_h} for a crop of {res}")
    return col[left:left + res], row[top:top + res], (res, res)


# --------------------------------------------------------------------------------------------------------------- folder datasets
def _open_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def _open_byte_plane(path, what):
    """An 8-bit single-channel image (mode L or P: the stored byte per pixel, as np.array(Image.open(...)) gives it)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "P"):
            raise ValueError(f"depthg_amd.data: {what} {path!r} has PIL mode {im.mode!r}; only 8-bit single-channel images (L, P) are taken")
        return np.asarray(im, dtype=np.uint8)


def _same_size(sample, names, index):
    h, w = sample.image.shape[:2]
    for plane, name in ((sample.label, names[0]), (sample.depth, names[1])):
        if isinstance(plane, np.ndarray) and plane.shape != (h, w):
            raise ValueError(f"depthg_amd.data: sample {index}: {name} is {plane.shape[1]}x{plane.shape[0]} but the image is {w}x{h} "
                             "(one crop serves a sample's planes: they must have one size)")
    return sample


class CroppedFolder:
    """CroppedDataset's layout (src/data.py:815-912): <root>/cropped/{name}_{crop}_crop_{ratio}[_{depth_type}]/{img,label,depth}/{split}/
    with {i}.jpg, {i}.png and {i}_{depth_type}.png.  label = stored byte - 1, mask = (label == -1) as bool; a `_plane` depth type gives
    a constant 255 depth map."""
    label_offset, mask_rule, label_dims = -1, ops.BATCH_MASK_BOOL_IGNORED, 3            # label (B,H,W), mask (B,1,H,W)

    def __init__(self, root, dataset_name, crop_type, crop_ratio, image_set, return_depth=False, depth_type="zoedepth"):
        self.data_dir, self.dataset_name, self.crop_type, self.split = root, dataset_name, crop_type, image_set
        self.nns_name = dataset_name
        self.n_classes = N_CLASSES.get(dataset_name)
        base = "{}_{}_crop_{}".format(dataset_name, crop_type, crop_ratio)
        if not ("zoedepth" in depth_type and dataset_name != "nyuv2"):                   # :825-833
            base += "_{}".format(depth_type)
        self.root = os.path.join(root, "cropped", base)
        self.img_dir, self.label_dir, self.depth_dir = (os.path.join(self.root, k, image_set) for k in ("img", "label", "depth"))
        if not os.path.isdir(self.img_dir):
            raise FileNotFoundError(f"depthg_amd.data: no image folder {self.img_dir!r}")
        if not os.path.isdir(self.label_dir):
            raise FileNotFoundError(f"depthg_amd.data: no label folder {self.label_dir!r} (the loader's label and mask come from it)")
        self.plane_depth = "plane" in depth_type
        self.depth_type = depth_type.replace("_plane", "")
        self.return_depth = bool(return_depth)
        self.has_labels = True
        self.num_images = len(os.listdir(self.img_dir))

    def __len__(self):
        return self.num_images

    def load(self, index):
        index = int(index)
        image = _open_rgb(os.path.join(self.img_dir, "{}.jpg".format(index)))
        label = _open_byte_plane(os.path.join(self.label_dir, "{}.png".format(index)), "label")
        depth = None
        if self.return_depth:
            depth = PLANE if self.plane_depth else \
                _open_byte_plane(os.path.join(self.depth_dir, "{}_{}.png".format(index, self.depth_type)), "depth map")
        return _same_size(Sample(image, label, depth), ("the label", "the depth map"), index)


class DirectoryFolder:
    """DirectoryDataset's layout (src/data.py:87-132): <root>/imgs/{split} and <root>/labels/{split}, both sorted, paired by position.
    The label is the stored byte, mask = (label > 0) as float32; without a labels folder the label is all -1.  No depth."""
    label_offset, mask_rule = 0, ops.BATCH_MASK_FLOAT_POSITIVE

    def __init__(self, root, image_set, name="directory", n_classes=None, crop_type=None):
        self.data_dir, self.split, self.nns_name, self.n_classes, self.crop_type = root, image_set, name, n_classes, crop_type
        self.img_dir, self.label_dir = os.path.join(root, "imgs", image_set), os.path.join(root, "labels", image_set)
        if not os.path.isdir(self.img_dir):
            raise FileNotFoundError(f"depthg_amd.data: no image folder {self.img_dir!r}")
        self.img_files = sorted(os.listdir(self.img_dir))
        if not self.img_files:
            raise FileNotFoundError(f"depthg_amd.data: no image in {self.img_dir!r}")
        self.has_labels = os.path.exists(os.path.join(root, "labels"))
        self.label_files = sorted(os.listdir(self.label_dir)) if self.has_labels else None
        if self.has_labels and len(self.label_files) != len(self.img_files):
            raise ValueError(f"depthg_amd.data: {len(self.img_files)} images in {self.img_dir!r} but {len(self.label_files)} labels in "
                             f"{self.label_dir!r}")
        self.label_dims = 4 if self.has_labels else 3      # label and mask (B,1,H,W) from files, (B,H,W) when filled with -1 (:126)
        self.return_depth = False

    def __len__(self):
        return len(self.img_files)

    def load(self, index):
        index = int(index)
        image = _open_rgb(os.path.join(self.img_dir, self.img_files[index]))
        label = _open_byte_plane(os.path.join(self.label_dir, self.label_files[index]), "label") if self.has_labels else None
        return _same_size(Sample(image, label, None), ("the label", "the depth map"), index)


# --------------------------------------------------------------------------------------------------------------- one batch
def _sample_records(dataset, sample, want_depth):
    """[(kind, plane or None)] of one sample: what the launch writes for it."""
    recs = [(ops.BATCH_IMAGE, sample.image)]
    recs.append((ops.BATCH_LABEL, sample.label) if sample.label is not None else (ops.BATCH_LABEL_FILL, None))
    if want_depth:
        if sample.depth is None:
            raise ValueError("depthg_amd.data: depth was asked for but the dataset returns none (return_depth=False, or a folder without depth)")
        recs.append((ops.BATCH_DEPTH_PLANE, None) if isinstance(sample.depth, str) else (ops.BATCH_DEPTH, sample.depth))
    return recs


def pack_batch(dataset, samples, tables, out_size, want_depth, pin=True):
    """(packed, records, tables): the decoded planes of `samples` back to back in one uint8 buffer (pinned when `pin` and a GPU is
    there), one int32 record of 8 words per output plane group (include/depthg_corr.h lists the words) and the int32 table
    (N, W + H) of `tables` = [(xs, ys)] - what ops.batch_prep takes."""
    H, W = out_size
    groups = [_sample_records(dataset, s, want_depth) for s in samples]
    total = sum(p.size for g in groups for _, p in g if p is not None)
    pin = bool(pin) and torch.cuda.is_available()
    packed = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=pin)
    flat = packed.numpy()
    fill = -1 if not dataset.has_labels else dataset.label_offset
    records, offset = [], 0
    for n, g in enumerate(groups):
        for kind, plane in g:
            if plane is None:
                records.append([kind, n, 0, 0, 0, 0, fill, dataset.mask_rule])
                continue
            flat[offset:offset + plane.size] = plane.reshape(-1)
            low = offset & 0xFFFFFFFF                       # the low word as the int32 with those bits
            records.append([kind, n, low - (1 << 32) if low >= (1 << 31) else low, offset >> 32, plane.shape[1], plane.shape[0],
                            dataset.label_offset, dataset.mask_rule])
            offset += plane.size
    table = torch.empty((len(samples), W + H), dtype=torch.int32)
    for n, (xs, ys) in enumerate(tables):
        table[n, :W] = torch.from_numpy(np.array(xs, dtype=np.int32))          # (a copy: the cached axis tables are read-only)
        table[n, W:] = torch.from_numpy(np.array(ys, dtype=np.int32))
    return packed, torch.tensor(records, dtype=torch.int32), table


def _cpu_chain(dataset, sample, res, crop_type, offsets, want_depth):
    """The plain chain on one sample (src/utils.py:164-182 and the dataset's __getitem__): PIL's nearest resize and crop, then the
    torch CPU operations, in their order.  Returns (img (3,H,W) fp32, label (H,W) int64, mask (H,W), depth (H,W) fp32 or None)."""
    from PIL import Image
    h, w = sample.image.shape[:2]
    new_w, new_h = resized_size(w, h, res, crop_type)
    if crop_type is None:
        box = None
    else:
        top, left = (center_crop_offset(new_h, res), center_crop_offset(new_w, res)) if crop_type == "center" else offsets
        box = (left, top, left + res, top + res)

    def geometry(plane):
        im = Image.fromarray(plane).resize((new_w, new_h), Image.NEAREST)
        return np.asarray(im.crop(box) if box is not None else im).copy()

    mean, std = (torch.tensor(v, dtype=torch.float32).reshape(3, 1, 1) for v in (ops.IMAGENET_MEAN, ops.IMAGENET_STD))
    img = torch.from_numpy(geometry(sample.image)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)      # ToTensor
    img = img.sub(mean).div(std)                                                                                 # Normalize
    if sample.label is not None:
        label = torch.as_tensor(geometry(sample.label), dtype=torch.int64) + dataset.label_offset                # ToTargetTensor, :901
    else:
        label = torch.zeros(img.shape[1], img.shape[2], dtype=torch.int64) - 1                                   # :126
    mask = (label == -1) if dataset.mask_rule == ops.BATCH_MASK_BOOL_IGNORED else (label > 0).to(torch.float32)  # :902, :128
    depth = None
    if want_depth:
        if sample.depth is None:
            raise ValueError("depthg_amd.data: depth was asked for but the dataset returns none (return_depth=False, or a folder without depth)")
        if isinstance(sample.depth, str):
            depth = torch.ones(img.shape[1], img.shape[2], dtype=torch.float32) * 255                            # :897-898
        else:
            depth = torch.as_tensor(geometry(sample.depth), dtype=torch.int64).float()                           # :894-895
    return img, label, mask, depth


def prepare_samples(dataset, samples, res, crop_type, device, want_depth, generator=None, offsets=None):
    """img (N,3,H,W), label (N,H,W), mask (N,H,W), depth (N,H,W) or None of the decoded `samples` on `device`: one dg_batch_prep launch on
    a GPU, the plain chain per sample on the CPU.  Random crops draw their offsets here, sample by sample, from `generator` (torch's
    CPU generator; None: the global one) unless `offsets` = [(top, left)] gives them."""
    device = torch.device(device)
    if offsets is None:
        offsets = [None] * len(samples)
        if crop_type == "random":
            sizes = [resized_size(s.image.shape[1], s.image.shape[0], res, crop_type) for s in samples]
            offsets = [draw_random_crop(nw, nh, res, generator) for nw, nh in sizes]
    if device.type != "cuda":
        rows = [_cpu_chain(dataset, s, res, crop_type, o, want_depth) for s, o in zip(samples, offsets)]
        img, label, mask = (torch.stack([r[k] for r in rows]) for k in range(3))
        return img, label, mask, (torch.stack([r[3] for r in rows]) if want_depth else None)
    tables, out_size = [], None
    for s, o in zip(samples, offsets):
        xs, ys, out_size = loader_index_tables(s.image.shape[1], s.image.shape[0], res, crop_type, o)
        tables.append((xs, ys))
    packed, records, table = pack_batch(dataset, samples, tables, out_size, want_depth)
    out = ops.batch_prep(packed, records, table, out_size, device=device, mean=ops.IMAGENET_MEAN, std=ops.IMAGENET_STD)
    return out["img"], out["label"], out["mask"], out.get("depth")


def _decode_samples(dataset, indices, threads):
    """dataset.load of every index, in a pool of `threads` threads (0: in the caller's thread)."""
    if threads == 0 or len(indices) < 2:
        return [dataset.load(i) for i in indices]
    with ThreadPoolExecutor(max_workers=min(threads, len(indices))) as pool:
        return list(pool.map(dataset.load, indices))


class ContrastiveBatches:
    """The batches `UnsupervisedSegmenter.training_step` / `validation_step` read, as the reference's DataLoader over
    ContrastiveSegDataset collates them (src/data.py:1073-1141): ind (B,), img (B,3,H,W), label, mask, depth (B,1,H,W) and, with
    `pos`, img_pos, ind_pos, depth_pos, label_pos, mask_pos of each sample's kNN positive - drawn from columns 1 .. cfg.num_neighbors
    of the table at knn.nns_path(...) (a missing file is the reference's ValueError).  The sample and its positive go through ONE
    dg_batch_prep launch; on a CPU `device` the plain chain runs instead.  `generator`: torch CPU generator of the shuffle and of the
    random crops (None: the global one).  Decoding runs in a pool of min(num_workers, 16) threads (0: in the caller's thread).  The
    last batch may be short (DataLoader's drop_last=False).  No img_aug / coord_aug: cfg.dg_gpu_augment makes them in the step."""

    def __init__(self, dataset, cfg, image_set, res, loader_crop_type, batch_size, shuffle=False, generator=None, num_workers=0,
                 pos=True, return_depth=None, device=None, feature_cache=None, sample_cache=None):
        self.dataset, self.cfg, self.image_set, self.res, self.loader_crop_type = dataset, cfg, image_set, int(res), loader_crop_type
        self.batch_size, self.shuffle, self.generator, self.pos = int(batch_size), bool(shuffle), generator, bool(pos)
        if self.batch_size < 1:
            raise ValueError(f"depthg_amd.data: batch_size={batch_size}")
        resized_size(1, 1, self.res, loader_crop_type)                  # (refuses an unknown cropper before anything is read)
        self.return_depth = bool(dataset.return_depth if return_depth is None else return_depth)
        self.threads = _decode_threads(num_workers)
        self.device = torch.device(_default_device(device))
        self.num_neighbors = int(getattr(cfg, "num_neighbors", 7))
        self.nns = None
        if self.pos:
            path = knn.nns_path(dataset.data_dir, cfg.model_type, dataset.nns_name, image_set, getattr(dataset, "crop_type", None),
                                getattr(cfg, "res", self.res))
            self.nns = knn.load_nns(path, len(dataset))
        # feature_cache.FeatureCache of this dataset's images (build_feature_cache): each batch then also carries the frozen backbone's
        # `image_feat` of its samples and `image_feat_pos` of their positives, gathered in one launch from the indices while they are
        # still on the host.  img / img_pos stay in the batch (the CRF and augmentation terms read them).  Without positives
        # (pos=False: a val split, whose cache train.val_feature_cache builds) the batch carries `image_feat` alone, from one launch
        # over the one index list - the short last batch included.
        self.feature_cache = feature_cache
        if feature_cache is not None:
            if loader_crop_type == "random":
                raise ValueError("depthg_amd.data: a feature cache holds the features of ONE view of every image; with loader_crop_type = "
                                 "'random' the view changes with every draw; use 'center' or None, or run without the cache")
            if feature_cache.n_images != len(dataset) or feature_cache.device != self.device:
                raise ValueError(f"depthg_amd.data: the feature cache holds {feature_cache.n_images} images on {feature_cache.device}, the "
                                 f"pipeline reads {len(dataset)} on {self.device}")

        # sample_cache.SampleCache of this dataset's images under this loader transform (build_sample_cache): img / label / mask / depth of
        # a batch and its positives then come from one gather launch over the cached bytes - nothing is decoded, packed or uploaded.
        self.sample_cache = sample_cache
        if sample_cache is not None:
            if loader_crop_type == "random":
                raise ValueError("depthg_amd.data: a sample cache holds the bytes of ONE view of every image; with loader_crop_type = "
                                 "'random' the view changes with every draw")
            if sample_cache.n_images != len(dataset) or sample_cache.device != self.device:
                raise ValueError(f"depthg_amd.data: the sample cache holds {sample_cache.n_images} images on {sample_cache.device}, the "
                                 f"pipeline reads {len(dataset)} on {self.device}")
            if (sample_cache.H, sample_cache.W) != (self.res, self.res) or sample_cache.has_labels != bool(dataset.has_labels) or \
                    (self.return_depth and not sample_cache.with_depth) or sample_cache.mask_rule != dataset.mask_rule or \
                    (dataset.has_labels and sample_cache.label_offset != dataset.label_offset):
                raise ValueError(f"depthg_amd.data: the sample cache ({sample_cache.H} x {sample_cache.W}, has_labels={sample_cache.has_labels}, "
                                 f"with_depth={sample_cache.with_depth}) was not built for this pipeline (res {self.res}, "
                                 f"has_labels={bool(dataset.has_labels)}, return_depth={self.return_depth}): build_sample_cache makes one that fits")

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _decode(self, indices):
        return _decode_samples(self.dataset, indices, self.threads)

    def _shape(self, t, dims):
        return t.unsqueeze(1) if dims == 4 else t

    def batch_of(self, inds):
        """The dictionary of the samples `inds` (and their positives, drawn here)."""
        inds = [int(i) for i in inds]
        B = len(inds)
        inds_pos = [knn.pick_positive(self.nns, i, self.num_neighbors) for i in inds] if self.pos else []
        if self.sample_cache is not None:
            img, label, mask, depth = self.sample_cache.gather(inds, inds_pos if self.pos else None)
        else:
            samples = self._decode(inds + inds_pos)
            img, label, mask, depth = prepare_samples(self.dataset, samples, self.res, self.loader_crop_type, self.device, self.return_depth,
                                                      self.generator)
        ld = self.dataset.label_dims
        label = self._shape(label, ld)
        mask = mask.unsqueeze(1) if (ld == 4 or self.dataset.mask_rule == ops.BATCH_MASK_BOOL_IGNORED) else mask
        batch = {"ind": torch.tensor(inds, dtype=torch.int64), "img": img[:B], "label": label[:B], "mask": mask[:B]}
        if self.return_depth:
            batch["depth"] = depth[:B].unsqueeze(1)
        if self.pos:
            batch.update({"img_pos": img[B:], "ind_pos": torch.tensor(inds_pos, dtype=torch.int64), "label_pos": label[B:], "mask_pos": mask[B:]})
            if self.return_depth:
                batch["depth_pos"] = depth[B:].unsqueeze(1)
        if self.feature_cache is not None and self.pos:
            batch["image_feat"], batch["image_feat_pos"] = self.feature_cache.gather(inds, inds_pos)
        elif self.feature_cache is not None:
            batch["image_feat"] = self.feature_cache.gather(inds)
        return batch

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        for i in range(0, n, self.batch_size):
            yield self.batch_of(order[i:i + self.batch_size])


# --------------------------------------------------------------------------------------------------------------- offline table
def precompute_knns(net, dataset, cfg, res, image_set, crop_type, batch_size=None, num_workers=0, device=None, n_batches=64):
    """src/precompute_knns.py:15-21, 85-115: centre-cropped batches of the whole dataset (through dg_batch_prep), `net`'s first output
    pooled and normalised - F.normalize(feats.mean([2, 3]), dim=1) -, knn.nearest_neighbors, knn.save_nns at knn.nns_path(data_dir,
    cfg.model_type, name, image_set, crop_type, res).  The table holds min(30, n_images) columns (the reference's topk(30) needs 30
    images).  Returns the path."""
    if batch_size is None:
        batch_size = 128 if cfg.model_type == "vit_small" else 64                 # :90
    batches = ContrastiveBatches(dataset, cfg, image_set, res, "center", batch_size, shuffle=False, num_workers=num_workers, pos=False,
                                 return_depth=False, device=device)
    if batches.device.type != "cuda":
        raise RuntimeError("depthg_amd.data: precompute_knns runs on the GPU (knn.nearest_neighbors has no CPU path)")
    was_training = net.training
    net.eval()
    feats = []
    try:
        with torch.no_grad():
            for batch in batches:
                feats.append(F.normalize(net(batch["img"])[0].mean([2, 3]), dim=1))
    finally:
        net.train(was_training)
    normed = torch.cat(feats, dim=0).contiguous()
    table = knn.nearest_neighbors(normed, k=min(knn.NNS_K, normed.shape[0]), n_batches=n_batches)
    path = knn.nns_path(dataset.data_dir, cfg.model_type, dataset.nns_name, image_set, crop_type, res)
    knn.save_nns(path, table)
    return path


# --------------------------------------------------------------------------------------------------------------- feature cache
def feature_cache_meta(cfg, dataset, res, crop_type, image_set=None, mirrored=False):
    """What the cached features of `dataset` depend on (FeatureCache.meta): the backbone, the view, the images.  crop_type: the
    LOADER's crop (the dataset's own crop is part of its name).  `image_set`: the split, named in the metadata of every cache but the
    train split's (whose files carry no such key: a file without it never matches a request that names one).  `mirrored`: the features
    of the horizontally mirrored images (evaluate_batch's flip pass)."""
    meta = {"model_type": str(getattr(cfg, "model_type", "vit_small")), "dino_patch_size": int(cfg.dino_patch_size),
            "dino_feat_type": str(getattr(cfg, "dino_feat_type", "feat")), "res": int(res), "loader_crop_type": crop_type,
            "dataset_name": "{}_{}".format(dataset.nns_name, getattr(dataset, "crop_type", None)), "n_images": len(dataset),
            "pretrained_weights": getattr(cfg, "pretrained_weights", None)}
    if image_set is not None:
        meta["split"] = str(image_set)
    if mirrored:
        meta["mirrored"] = True
    return meta


def feature_cache_path(data_dir, meta, image_set, dtype):
    """<data_dir>/feature_cache_<meta>.pt"""
    from .feature_cache import as_dtype
    name = "feature_cache_{model_type}_{dino_feat_type}{dino_patch_size}_{dataset_name}_{image_set}_{loader_crop_type}_{res}_{n_images}_{dtype}.pt".format(
        image_set=image_set, dtype=("mirrored_" if meta.get("mirrored") else "") + str(as_dtype(dtype)).replace("torch.", ""), **meta)
    return os.path.join(data_dir, name)


def build_feature_cache(net, dataset, cfg, res, crop_type, dtype=torch.float32, device=None, batch_size=None, num_workers=0,
                        sample_cache=None, image_set=None, mirrored=False):
    """A feature_cache.FeatureCache of `dataset`: one pass over the split in index order through `prepare_samples` with the loader
    transform (res, crop_type - the pipeline's loader_crop_type), `net._backbone(img)` under no_grad with the backbone in eval mode
    (what forward() runs, src/modules.py:93-120), one `put` per batch.  The pass --precompute-knns makes over the same images pools
    and drops these maps; this one keeps them.  Refused: crop_type "random" (the features would depend on the draw) and cfg.arch
    "dino_depth" (the depth-guided featurizer mixes the depth map in behind the backbone: out of scope for the cache).
    `sample_cache`: a sample_cache.SampleCache of the same split and transform to fill from the samples this pass decodes anyway, so
    that a run that wants both caches decodes the split once.  `image_set`: the split the metadata name (feature_cache_meta; None: the
    train split's form).  `mirrored`: the backbone runs on img.flip(dims=[3]) - the features evaluate_batch(flip=True) reads as
    `image_feat_flip` (a mirrored feature map is not the feature map of the mirrored image); the sample cache still gets the images
    as they are."""
    from .feature_cache import FeatureCache
    _refuse_random_crop(crop_type, "depthg_amd.data: build_feature_cache", "features")
    if getattr(cfg, "arch", "dino") == "dino_depth" or not hasattr(net, "forward_pair_features") or not hasattr(net, "_backbone"):
        raise ValueError("depthg_amd.data: build_feature_cache serves cfg.arch = 'dino' (a FrozenBackboneFeaturizer); the depth-guided "
                         "featurizer of arch 'dino_depth' is out of scope for the feature cache")
    resized_size(1, 1, res, crop_type)
    device = torch.device(_default_device(device))
    if batch_size is None:
        batch_size = 128 if cfg.model_type == "vit_small" else 64
    threads = _decode_threads(num_workers)
    n = len(dataset)
    cache = None
    net.model.eval()
    with torch.no_grad():
        for i in range(0, n, int(batch_size)):
            inds = list(range(i, min(i + int(batch_size), n)))
            samples = _decode_samples(dataset, inds, threads)
            if sample_cache is not None:
                sample_cache.put(inds, samples, res, crop_type)
            img = prepare_samples(dataset, samples, res, crop_type, device, False)[0]
            image_feat = net._backbone(img.flip(dims=[3]) if mirrored else img)[0]
            if cache is None:
                cache = FeatureCache(n, *image_feat.shape[1:], dtype=dtype, device=device,
                                     meta=feature_cache_meta(cfg, dataset, res, crop_type, image_set, mirrored))
            cache.put(inds, image_feat)
    if cache is None:
        raise ValueError("depthg_amd.data: build_feature_cache on an empty dataset")
    return cache


# --------------------------------------------------------------------------------------------------------------- sample cache
def sample_cache_meta(dataset, image_set, res, crop_type, want_depth):
    """What the cached bytes of `dataset` depend on (SampleCache.meta): the images, the split, the view, the planes.  crop_type: the
    LOADER's crop (the dataset's own crop is part of its name)."""
    return {"dataset_name": "{}_{}".format(dataset.nns_name, getattr(dataset, "crop_type", None)), "split": str(image_set), "res": int(res),
            "loader_crop_type": crop_type, "n_images": len(dataset), "has_labels": bool(dataset.has_labels),
            "depth_type": (("plane_" if getattr(dataset, "plane_depth", False) else "") + str(getattr(dataset, "depth_type", None)))
            if want_depth else None}


def sample_cache_path(data_dir, meta):
    """<data_dir>/sample_cache_<meta>.pt"""
    name = "sample_cache_{dataset_name}_{split}_{loader_crop_type}_{res}_{n_images}_{depth_type}_{labels}.pt".format(
        labels="labels" if meta["has_labels"] else "nolabels", **meta)
    return os.path.join(data_dir, name)


def new_sample_cache(dataset, image_set, res, crop_type, want_depth, device):
    """An empty sample_cache.SampleCache for `dataset` under the loader transform (res, crop_type): what build_sample_cache fills, and
    what build_feature_cache(sample_cache=...) takes to fill on its own pass."""
    from .sample_cache import SampleCache
    _refuse_random_crop(crop_type, "depthg_amd.data: a sample cache", "bytes")
    resized_size(1, 1, res, crop_type)
    if len(dataset) < 1:
        raise ValueError("depthg_amd.data: a sample cache of an empty dataset")
    return SampleCache(len(dataset), int(res), int(res), dataset.has_labels, want_depth, dataset.label_offset if dataset.has_labels else 0, -1,
                       dataset.mask_rule, device=device, meta=sample_cache_meta(dataset, image_set, res, crop_type, want_depth))


def fill_sample_cache(cache, dataset, res, crop_type, num_workers=0, batch_size=64):
    """Put every row of `cache` that has not been put yet, in index order: decoding in the thread pool (min(num_workers, 16) threads),
    one `put` - one launch - per `batch_size` images."""
    threads = _decode_threads(num_workers)
    missing = np.flatnonzero(~cache.filled).tolist()
    for i in range(0, len(missing), int(batch_size)):
        inds = missing[i:i + int(batch_size)]
        cache.put(inds, _decode_samples(dataset, inds, threads), res, crop_type)
    return cache


def build_sample_cache(dataset, cfg, res, crop_type, want_depth=None, device=None, num_workers=0, image_set=None, batch_size=64):
    """A sample_cache.SampleCache of `dataset` under the loader transform (res, crop_type): one decoding pass over the split in index
    order (fill_sample_cache).  `want_depth`: None takes the dataset's return_depth.  Refused: crop_type "random" (the bytes would
    depend on the draw).  (`cfg` is not read: the transform is all the bytes depend on.)"""
    want_depth = bool(dataset.return_depth if want_depth is None else want_depth)
    cache = new_sample_cache(dataset, image_set if image_set is not None else getattr(dataset, "split", None), res, crop_type, want_depth, device)
    return fill_sample_cache(cache, dataset, res, crop_type, num_workers, batch_size)
