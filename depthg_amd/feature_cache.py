"""FeatureCache: the frozen backbone's `image_feat` of every train image, computed once and read back per batch.

The backbone of DinoFeaturizer is frozen, runs in eval mode under no_grad and draws no random numbers (src/modules.py:90-137), and with
`loader_crop_type = "center"` every train image and every kNN positive reaches it through a deterministic transform: the `image_feat`
of train image i, which the step's two featurizer passes recompute in every epoch (src/train_segmentation.py:194-212), is one tensor.
The cache stores it as an (n_images, C h w) table of float32, float16 or bfloat16 on the device - `put` narrows with torch's rounding,
`gather` widens exactly - and hands a batch and its positives back as ONE fp32 allocation from ONE launch (ops.feature_cache_put /
ops.feature_cache_gather over k_fc_put / k_fc_gather of dg_feat_cache.hip), laid out as the head's paired pass takes its two maps.
data.build_feature_cache fills one, data.ContrastiveBatches(feature_cache=...) puts `image_feat` / `image_feat_pos` into its batches,
and with cfg.dg_feature_cache set training_step starts from them (FrozenBackboneFeaturizer.forward_features / forward_pair_features)
instead of running the backbone.

On a CPU `device` the class is plain torch - index_copy_, index_select and casts: the statement the kernels are tested against.
A cache that does not fit on the card is out of scope: construction fails with torch's out-of-memory error, the needed bytes named.
"""
import numpy as np
import torch

from . import ops

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def as_dtype(dtype):
    """torch.float32 / float16 / bfloat16 from the dtype or its name (the train command's --feature-cache value)."""
    dt = DTYPES.get(dtype, dtype) if isinstance(dtype, str) else dtype
    if dt not in DTYPES.values():
        raise ValueError(f"depthg_amd: a feature cache stores float32, float16 or bfloat16, not {dtype!r}")
    return dt


class FeatureCache:
    """FeatureCache(n_images, C, h, w, dtype=torch.float32, device=...): row i = image_feat (C, h, w) of image i.
        put(indices, image_feat)     store image_feat (n, C, h, w) as rows `indices`
        gather(ind, ind_pos=None)    (B, C, h, w) fp32 of rows `ind` - with `ind_pos` two such tensors, views of one (2B, C, h, w) allocation
        filled                       host-side bool array (n_images,): the rows put so far
        nbytes                       bytes of the table
        meta                         what the features depend on: model_type, dino_patch_size, dino_feat_type, res, loader_crop_type,
                                     dataset_name, n_images (set by data.build_feature_cache; `n_images` from the start)
        save(path) / FeatureCache.load(path, device, expect_meta)
    Indices are CPU int64 tensors or sequences of ints and are checked on the host before anything is launched: an index outside
    [0, n_images) is an IndexError; a duplicate inside one `put`, a `put` whose count differs from image_feat's, and a `gather` of a
    row that was never put are ValueErrors - each names the offending value.  `gather` may repeat an index, inside a list or between them."""

    def __init__(self, n_images, C, h, w, dtype=torch.float32, device=None, meta=None):
        self.n_images, self.shape = int(n_images), (int(C), int(h), int(w))
        if self.n_images < 1 or min(self.shape) < 1:
            raise ValueError(f"depthg_amd: FeatureCache of {n_images} images of {C} x {h} x {w} features")
        self.dtype = as_dtype(dtype)
        if device is None:
            device = "cuda:0" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.row = self.shape[0] * self.shape[1] * self.shape[2]
        need = self.n_images * self.row * torch.empty((), dtype=self.dtype).element_size()
        try:
            self.data = torch.empty((self.n_images, self.row), dtype=self.dtype, device=self.device)
        except torch.OutOfMemoryError as e:
            raise torch.OutOfMemoryError(f"depthg_amd: a {self.dtype} feature cache of {self.n_images} images of {self.shape} needs "
                                         f"{need} bytes on {self.device}: {e}") from e
        self.filled = np.zeros(self.n_images, dtype=bool)
        self.meta = {"n_images": self.n_images, **(meta or {})}

    @property
    def nbytes(self):
        return self.data.numel() * self.data.element_size()

    def _indices(self, indices, name):
        """`indices` as a numpy int64 array, every value inside [0, n_images).  (numpy: the checks of a batch cost a few microseconds.)"""
        if isinstance(indices, torch.Tensor):
            if indices.is_cuda or indices.is_floating_point() or indices.dtype == torch.bool or indices.dim() != 1:
                raise ValueError(f"depthg_amd: FeatureCache wants `{name}` as a 1-d CPU integer tensor or a sequence of ints, got "
                                 f"{tuple(indices.shape)} {indices.dtype} on {indices.device}")
            arr = indices.to(torch.int64).numpy()
        else:
            arr = np.asarray(indices)
            if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
                raise ValueError(f"depthg_amd: FeatureCache wants `{name}` as a 1-d CPU integer tensor or a sequence of ints, got an array "
                                 f"of shape {arr.shape} and type {arr.dtype}")
            arr = arr.astype(np.int64, copy=False)
        if arr.size and (arr.min() < 0 or arr.max() >= self.n_images):
            bad = arr[(arr < 0) | (arr >= self.n_images)]
            raise IndexError(f"depthg_amd: FeatureCache `{name}` holds {int(bad[0])}, outside [0, {self.n_images})")
        return arr

    def put(self, indices, image_feat):
        idx = self._indices(indices, "indices")
        n = idx.size
        if image_feat.dim() != 4 or tuple(image_feat.shape[1:]) != self.shape or image_feat.shape[0] != n:
            raise ValueError(f"depthg_amd: FeatureCache.put of {n} indices wants image_feat ({n}, {', '.join(map(str, self.shape))}), got "
                             f"{tuple(image_feat.shape)}")
        values, counts = np.unique(idx, return_counts=True)
        if values.size != n:
            raise ValueError(f"depthg_amd: FeatureCache.put names row {int(values[counts > 1][0])} more than once in one call")
        if image_feat.device != self.device:
            raise ValueError(f"depthg_amd: FeatureCache.put: image_feat lives on {image_feat.device}, the cache on {self.device}")
        if n == 0:
            return
        rows = torch.from_numpy(np.ascontiguousarray(idx))
        if self.device.type == "cuda":
            ops.feature_cache_put(self.data, rows.to(self.device), image_feat)
        else:
            self.data.index_copy_(0, rows, image_feat.detach().to(torch.float32).reshape(n, self.row).to(self.dtype))
        self.filled[idx] = True

    def gather(self, ind, ind_pos=None):
        lists = [self._indices(ind, "ind")] + ([self._indices(ind_pos, "ind_pos")] if ind_pos is not None else [])
        n = lists[0].size
        if ind_pos is not None and lists[1].size != n:
            raise ValueError(f"depthg_amd: FeatureCache.gather: {n} indices and {lists[1].size} positives")
        both = np.concatenate(lists) if ind_pos is not None else np.ascontiguousarray(lists[0])
        if not self.filled[both].all():
            for idx, name in zip(lists, ("ind", "ind_pos")):
                empty = idx[~self.filled[idx]]
                if empty.size:
                    raise ValueError(f"depthg_amd: FeatureCache.gather: row {int(empty[0])} of `{name}` was never put")
        rows = torch.from_numpy(both)
        if self.device.type == "cuda":
            on_dev = rows.to(self.device)                      # one upload for both lists
            out = ops.feature_cache_gather(self.data, on_dev[:n], on_dev[n:] if ind_pos is not None else None)
        else:
            out = self.data.index_select(0, rows).to(torch.float32)
        out = out.reshape((both.size,) + self.shape)
        return out if ind_pos is None else (out[:n], out[n:])

    def check_meta(self, expect_meta):
        """ValueError naming the keys of `expect_meta` this cache's metadata lacks or holds another value for."""
        differ = [k for k, v in expect_meta.items() if k not in self.meta or self.meta[k] != v]
        if differ:
            raise ValueError("depthg_amd: the feature cache was built for other settings: " +
                             ", ".join(f"{k} = {self.meta.get(k)!r} (expected {expect_meta[k]!r})" for k in differ))

    def save(self, path):
        torch.save({"meta": dict(self.meta), "shape": list(self.shape), "dtype": str(self.dtype).replace("torch.", ""),
                    "filled": torch.from_numpy(self.filled.copy()), "data": self.data.cpu()}, path)

    @classmethod
    def load(cls, path, device=None, expect_meta=None):
        """The cache `save` wrote, on `device`.  `expect_meta`: a dict every key of which must be in the file's metadata with that value."""
        blob = torch.load(path, map_location="cpu", weights_only=True)
        cache = cls(int(blob["meta"]["n_images"]), *blob["shape"], dtype=blob["dtype"], device=device, meta=blob["meta"])
        if expect_meta is not None:
            cache.check_meta(expect_meta)
        if tuple(blob["data"].shape) != tuple(cache.data.shape) or blob["data"].dtype != cache.dtype:
            raise ValueError(f"depthg_amd: {path}: the stored table {tuple(blob['data'].shape)} {blob['data'].dtype} is not the "
                             f"{tuple(cache.data.shape)} {cache.dtype} its header describes")
        cache.data.copy_(blob["data"])
        cache.filled[:] = blob["filled"].numpy()
        return cache
