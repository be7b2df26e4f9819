"""SampleCache: the loader's output bytes of every image of a split, kept on the device and read back per batch.

With a deterministic `loader_crop_type` ("center" or None) the loader transform (src/utils.py:164-182: nearest resize, crop) selects
the same bytes of an image, its label and its depth map in every epoch, and everything the datasets form from them - ToTensor and
Normalize, `label - 1`, the masks, the depth as float (src/data.py:894-902, :126-128) - is arithmetic on those bytes.  The cache
stores them once as a uint8 tensor (n_images, planes, H, W) at the loader's OUTPUT size, planes R, G, B, then the label if the dataset
has labels, then the depth if it is wanted: 251 KB per image at 224 x 224 with all five.  `put` writes rows from decoded samples with
one launch (ops.sample_cache_put, k_sc_put of dg_sample_cache.hip: k_batch_prep's tile prologue and gather, the bytes stored as they
are), `gather` hands a batch and its positives back as img / label / mask / depth in the step's dtypes from ONE launch
(ops.sample_cache_gather, k_sc_gather) - no file, no decoder, no pinned buffer, no upload but the indices.  data.build_sample_cache fills one and
data.ContrastiveBatches(sample_cache=...) serves its batches from it.

On a CPU `device` the class is plain torch - index_copy_ / index_select on the byte tensor, then the operations of data._cpu_chain in
their order: the statement the kernels are tested against.  A cache that does not fit on the card is out of scope: construction fails
with torch's out-of-memory error, the needed bytes named.
"""
import numpy as np
import torch

from . import ops
from .row_cache import RowCache


class SampleCache(RowCache):
    """SampleCache(n_images, H, W, has_labels, with_depth, label_offset, fill, mask_rule, device, meta=None): row i = the planes of image i.
        has_labels, with_depth       whether a row carries a label plane / a depth plane
        label_offset, fill           label = byte + label_offset; without a label plane the label is the constant `fill`
        mask_rule                    ops.BATCH_MASK_BOOL_IGNORED (bool label == -1) or ops.BATCH_MASK_FLOAT_POSITIVE (fp32 label > 0)
        put(indices, samples, res, crop_type)   store the loader transform's bytes of the decoded data.Sample `samples` as rows `indices`
        put_tables(indices, samples, tables)    the same from given index tables
        gather(inds, inds_pos=None)  (img (n,3,H,W) fp32, label (n,H,W) int64, mask (n,H,W), depth (n,H,W) fp32 or None) of rows `inds`;
                                     with `inds_pos` n = 2 len(inds): the batch first, the positives behind it, one allocation each
        filled                       host-side bool array (n_images,): the rows put so far
        nbytes                       bytes of the table
        meta                         what the bytes depend on (data.sample_cache_meta; `n_images` from the start)
        save(path) / SampleCache.load(path, device, expect_meta)
    Indices are CPU int64 tensors or sequences of ints, checked on the host before anything is launched: an index outside
    [0, n_images) is an IndexError; a duplicate inside one `put`, a count that differs from the samples', and a `gather` of a row that
    was never put are ValueErrors.  `gather` may repeat an index, inside a list or between them."""
    noun = "sample cache"

    def __init__(self, n_images, H, W, has_labels, with_depth, label_offset, fill, mask_rule, device=None, meta=None):
        self.H, self.W = int(H), int(W)
        if int(n_images) < 1 or self.H < 1 or self.W < 1:
            raise ValueError(f"depthg_amd: SampleCache of {n_images} images of {H} x {W}")
        if self.W % 4:
            raise ValueError(f"depthg_amd: SampleCache rows of width {W}: the kernels move four columns as one word, as dg_batch_prep does; "
                             "use a res that is a multiple of 4")
        if mask_rule not in (ops.BATCH_MASK_BOOL_IGNORED, ops.BATCH_MASK_FLOAT_POSITIVE):
            raise ValueError(f"depthg_amd: SampleCache: unknown mask rule {mask_rule!r}")
        self.has_labels, self.with_depth = bool(has_labels), bool(with_depth)
        self.label_offset, self.fill, self.mask_rule = int(label_offset), int(fill), int(mask_rule)
        self.planes = 3 + int(self.has_labels) + int(self.with_depth)
        self.label_plane = 3 if self.has_labels else None
        self.depth_plane = 3 + int(self.has_labels) if self.with_depth else None
        super().__init__(n_images, (self.planes, self.H, self.W), torch.uint8, device, meta,
                         f"a sample cache of {int(n_images)} images of {self.planes} planes of {self.H} x {self.W}")

    def put(self, indices, samples, res, crop_type):
        from . import data
        data._refuse_random_crop(crop_type, "depthg_amd: SampleCache.put", "bytes")
        tables = []
        for k, s in enumerate(samples):
            xs, ys, out_size = data.loader_index_tables(s.image.shape[1], s.image.shape[0], res, crop_type)
            if tuple(out_size) != (self.H, self.W):
                raise ValueError(f"depthg_amd: SampleCache.put: the loader transform (res {res}, crop {crop_type!r}) gives sample {k} "
                                 f"{out_size[0]} x {out_size[1]} pixels, the cache's rows hold {self.H} x {self.W}: every sample must "
                                 "come out at the cache's size (one res, crop 'center' or None)")
            tables.append((xs, ys))
        self.put_tables(indices, samples, tables)

    def put_tables(self, indices, samples, tables):
        """`put` with the index tables given: tables[k] = (xs[W], ys[H]), the source column of every output column and the source row of
        every output row of sample k (what data.loader_index_tables composes from a resize and a crop)."""
        from . import data
        idx = self._indices(indices, "indices")
        n = idx.size
        if len(samples) != n or len(tables) != n:
            raise ValueError(f"depthg_amd: SampleCache.put of {n} indices got {len(samples)} samples")
        self._check_unique(idx)
        for k, s, (xs, ys) in zip(idx, samples, tables):
            if (s.label is not None) != self.has_labels:
                raise ValueError(f"depthg_amd: SampleCache.put: sample {int(k)} " +
                                 ("carries a label but the cache has no label plane: build it with has_labels=True" if s.label is not None else
                                  "carries no label but the cache has a label plane: build it with has_labels=False"))
            if self.with_depth and s.depth is None:
                raise ValueError("depthg_amd: depth was asked for but the dataset returns none (return_depth=False, or a folder without depth)")
            h, w = s.image.shape[:2]
            if len(xs) != self.W or len(ys) != self.H or min(xs) < 0 or max(xs) >= w or min(ys) < 0 or max(ys) >= h:
                raise ValueError(f"depthg_amd: SampleCache.put: the tables of sample {int(k)} do not address {self.H} x {self.W} pixels inside "
                                 f"its {h} x {w} planes")
        if n == 0:
            return
        rows = torch.from_numpy(np.ascontiguousarray(idx))
        if self.device.type == "cuda":
            packed, records, table = data.pack_batch(self, samples, tables, (self.H, self.W), self.with_depth)
            ops.sample_cache_put(self.data, self.has_labels, self.with_depth, rows.to(self.device), packed, records, table)
        else:
            block = torch.empty((n, self.planes, self.H, self.W), dtype=torch.uint8)
            for k, (s, (xs, ys)) in enumerate(zip(samples, tables)):
                grid = np.ix_(np.asarray(ys), np.asarray(xs))
                block[k, :3] = torch.from_numpy(np.ascontiguousarray(s.image[grid].transpose(2, 0, 1)))
                if self.has_labels:
                    block[k, self.label_plane] = torch.from_numpy(np.ascontiguousarray(s.label[grid]))
                if self.with_depth:                                                                   # data.PLANE: src/data.py:897-898
                    block[k, self.depth_plane] = 255 if isinstance(s.depth, str) else torch.from_numpy(np.ascontiguousarray(s.depth[grid]))
            self.data.index_copy_(0, rows, block)
        self.filled[idx] = True

    def gather(self, inds, inds_pos=None):
        rows, _, idx_a, idx_b = self._gather_rows(inds, inds_pos, ("inds", "inds_pos"))
        if self.device.type == "cuda":
            out = ops.sample_cache_gather(self.data, self.has_labels, self.with_depth, idx_a, idx_b, label_offset=self.label_offset,
                                          fill=self.fill, mask_rule=self.mask_rule, mean=ops.IMAGENET_MEAN, std=ops.IMAGENET_STD)
            return out["img"], out["label"], out["mask"], out.get("depth")
        planes = self.data.index_select(0, rows)
        mean, std = (torch.tensor(v, dtype=torch.float32).reshape(1, 3, 1, 1) for v in (ops.IMAGENET_MEAN, ops.IMAGENET_STD))
        img = planes[:, :3].to(torch.float32).div(255).sub(mean).div(std)                            # ToTensor, Normalize
        if self.has_labels:
            label = planes[:, self.label_plane].to(torch.int64) + self.label_offset                  # ToTargetTensor, src/data.py:901
        else:
            label = torch.full((rows.numel(), self.H, self.W), self.fill, dtype=torch.int64)         # :126
        mask = (label == -1) if self.mask_rule == ops.BATCH_MASK_BOOL_IGNORED else (label > 0).to(torch.float32)
        depth = planes[:, self.depth_plane].to(torch.int64).float() if self.with_depth else None     # :894-898
        return img, label, mask, depth

    def _header(self):
        return {"H": self.H, "W": self.W, "has_labels": self.has_labels, "with_depth": self.with_depth, "label_offset": self.label_offset,
                "fill": self.fill, "mask_rule": self.mask_rule}

    @classmethod
    def _from_header(cls, blob, device):
        return cls(int(blob["meta"]["n_images"]), blob["H"], blob["W"], blob["has_labels"], blob["with_depth"], blob["label_offset"],
                   blob["fill"], blob["mask_rule"], device=device, meta=blob["meta"])

    def _table_text(self):
        return f"{tuple(self.data.shape)} uint8"
