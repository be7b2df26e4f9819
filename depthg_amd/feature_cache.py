"""FeatureCache: the frozen backbone's `image_feat` of every train image, computed once and read back per batch.

The backbone of DinoFeaturizer is frozen, runs in eval mode under no_grad and draws no random numbers (src/modules.py:90-137), and with
`loader_crop_type = "center"` every train image and every kNN positive reaches it through a deterministic transform: the `image_feat`
of train image i, which the step's two featurizer passes recompute in every epoch (src/train_segmentation.py:194-212), is one tensor.
The cache stores it as an (n_images, C h w) table of float32, float16 or bfloat16 on the device - `put` narrows with torch's rounding,
`gather` widens exactly - and hands a batch and its positives back as ONE fp32 allocation from ONE launch (ops.feature_cache_put /
ops.feature_cache_gather over k_fc_put / k_fc_gather of dg_feat_cache.hip), laid out as the head's paired pass takes its two maps.
data.build_feature_cache fills one, data.ContrastiveBatches(feature_cache=...) puts `image_feat` / `image_feat_pos` into its batches,
and with cfg.dg_feature_cache set training_step starts from them (FrozenBackboneFeaturizer.forward_features / forward_pair_features)
instead of running the backbone.  A second cache can hold the val split (train.val_feature_cache, cfg.dg_val_feature_cache):
data.ContrastiveBatches(pos=False, feature_cache=...) then puts `image_feat` alone into each val batch - `gather` with one index list,
still one launch - and validation_step / evaluate_batch start behind the backbone.

On a CPU `device` the class is plain torch - index_copy_, index_select and casts: the statement the kernels are tested against.
A cache that does not fit on the card is out of scope: construction fails with torch's out-of-memory error, the needed bytes named.
"""
import numpy as np
import torch

from . import ops
from .row_cache import RowCache

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def as_dtype(dtype):
    """torch.float32 / float16 / bfloat16 from the dtype or its name (the train command's --feature-cache value)."""
    dt = DTYPES.get(dtype, dtype) if isinstance(dtype, str) else dtype
    if dt not in DTYPES.values():
        raise ValueError(f"depthg_amd: a feature cache stores float32, float16 or bfloat16, not {dtype!r}")
    return dt


class FeatureCache(RowCache):
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
    noun = "feature cache"

    def __init__(self, n_images, C, h, w, dtype=torch.float32, device=None, meta=None):
        self.shape = (int(C), int(h), int(w))
        if int(n_images) < 1 or min(self.shape) < 1:
            raise ValueError(f"depthg_amd: FeatureCache of {n_images} images of {C} x {h} x {w} features")
        self.dtype = as_dtype(dtype)
        self.row = self.shape[0] * self.shape[1] * self.shape[2]
        super().__init__(n_images, (self.row,), self.dtype, device, meta, f"a {self.dtype} feature cache of {int(n_images)} images of {self.shape}")

    def put(self, indices, image_feat):
        idx = self._indices(indices, "indices")
        n = idx.size
        if image_feat.dim() != 4 or tuple(image_feat.shape[1:]) != self.shape or image_feat.shape[0] != n:
            raise ValueError(f"depthg_amd: FeatureCache.put of {n} indices wants image_feat ({n}, {', '.join(map(str, self.shape))}), got "
                             f"{tuple(image_feat.shape)}")
        self._check_unique(idx)
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
        rows, n, idx_a, idx_b = self._gather_rows(ind, ind_pos, ("ind", "ind_pos"))
        if self.device.type == "cuda":
            out = ops.feature_cache_gather(self.data, idx_a, idx_b)
        else:
            out = self.data.index_select(0, rows).to(torch.float32)
        out = out.reshape((rows.numel(),) + self.shape)
        return out if ind_pos is None else (out[:n], out[n:])

    def _header(self):
        return {"shape": list(self.shape), "dtype": str(self.dtype).replace("torch.", "")}

    @classmethod
    def _from_header(cls, blob, device):
        return cls(int(blob["meta"]["n_images"]), *blob["shape"], dtype=blob["dtype"], device=device, meta=blob["meta"])
