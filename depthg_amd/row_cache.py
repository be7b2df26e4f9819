"""RowCache: what FeatureCache and SampleCache share - a device table with one row per image of a split, the host-side record of the
rows put so far, the checks of an index list, the metadata and the file.  A subclass says what a row is (its shape and dtype), names
itself in the messages (`noun`; the class name comes from the class) and supplies the body of `put` and `gather` behind the shared
preambles."""
import numpy as np
import torch

from .data import _default_device


class RowCache:
    noun = "row cache"                                # the cache in words: "the feature cache was built for other settings"

    def __init__(self, n_images, row_shape, dtype, device, meta, what):
        """The table (n_images, *row_shape) of `dtype` on `device` (None: the first GPU, else the CPU).  `what`: the cache in words, for
        the out-of-memory error."""
        self.n_images = int(n_images)
        self.device = torch.device(_default_device(device))
        shape = (self.n_images,) + tuple(int(s) for s in row_shape)
        try:
            self.data = torch.empty(shape, dtype=dtype, device=self.device)
        except torch.OutOfMemoryError as e:
            need = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
            raise torch.OutOfMemoryError(f"depthg_amd: {what} needs {need} bytes on {self.device}: {e}") from e
        self.filled = np.zeros(self.n_images, dtype=bool)
        self.meta = {"n_images": self.n_images, **(meta or {})}

    @property
    def nbytes(self):
        return self.data.numel() * self.data.element_size()

    def _indices(self, indices, name):
        """`indices` as a numpy int64 array, every value inside [0, n_images).  (numpy: the checks of a batch cost a few microseconds.)"""
        who = type(self).__name__
        if isinstance(indices, torch.Tensor):
            if indices.is_cuda or indices.is_floating_point() or indices.dtype == torch.bool or indices.dim() != 1:
                raise ValueError(f"depthg_amd: {who} wants `{name}` as a 1-d CPU integer tensor or a sequence of ints, got "
                                 f"{tuple(indices.shape)} {indices.dtype} on {indices.device}")
            arr = indices.to(torch.int64).numpy()
        else:
            arr = np.asarray(indices)
            if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
                raise ValueError(f"depthg_amd: {who} wants `{name}` as a 1-d CPU integer tensor or a sequence of ints, got an array "
                                 f"of shape {arr.shape} and type {arr.dtype}")
            arr = arr.astype(np.int64, copy=False)
        if arr.size and (arr.min() < 0 or arr.max() >= self.n_images):
            bad = arr[(arr < 0) | (arr >= self.n_images)]
            raise IndexError(f"depthg_amd: {who} `{name}` holds {int(bad[0])}, outside [0, {self.n_images})")
        return arr

    def _check_unique(self, idx):
        """A `put` writes each of its rows once."""
        values, counts = np.unique(idx, return_counts=True)
        if values.size != idx.size:
            raise ValueError(f"depthg_amd: {type(self).__name__}.put names row {int(values[counts > 1][0])} more than once in one call")

    def _gather_rows(self, ind, ind_pos, names):
        """The preamble of `gather`: both lists checked, of one length, every row put.  Returns (rows, n, idx_a, idx_b): the CPU int64
        tensor of both lists, the length of one, and on a GPU their device copies from one upload (idx_b None without `ind_pos`)."""
        lists = [self._indices(ind, names[0])] + ([self._indices(ind_pos, names[1])] if ind_pos is not None else [])
        n = lists[0].size
        if ind_pos is not None and lists[1].size != n:
            raise ValueError(f"depthg_amd: {type(self).__name__}.gather: {n} indices and {lists[1].size} positives")
        both = np.concatenate(lists) if ind_pos is not None else np.ascontiguousarray(lists[0])
        if not self.filled[both].all():
            for idx, name in zip(lists, names):
                empty = idx[~self.filled[idx]]
                if empty.size:
                    raise ValueError(f"depthg_amd: {type(self).__name__}.gather: row {int(empty[0])} of `{name}` was never put")
        rows = torch.from_numpy(both)
        if self.device.type != "cuda":
            return rows, n, None, None
        on_dev = rows.to(self.device)                          # one upload for both lists
        return rows, n, on_dev[:n], (on_dev[n:] if ind_pos is not None else None)

    def check_meta(self, expect_meta):
        """ValueError naming the keys of `expect_meta` this cache's metadata lacks or holds another value for."""
        differ = [k for k, v in expect_meta.items() if k not in self.meta or self.meta[k] != v]
        if differ:
            raise ValueError(f"depthg_amd: the {self.noun} was built for other settings: " +
                             ", ".join(f"{k} = {self.meta.get(k)!r} (expected {expect_meta[k]!r})" for k in differ))

    def _header(self):
        """The constructor's arguments as `save` stores them beside meta, filled and data."""
        raise NotImplementedError

    @classmethod
    def _from_header(cls, blob, device):
        """An empty cache from what `save` stored."""
        raise NotImplementedError

    def _table_text(self):
        return f"{tuple(self.data.shape)} {self.data.dtype}"

    def save(self, path):
        torch.save({"meta": dict(self.meta), **self._header(), "filled": torch.from_numpy(self.filled.copy()), "data": self.data.cpu()}, path)

    @classmethod
    def load(cls, path, device=None, expect_meta=None):
        """The cache `save` wrote, on `device`.  `expect_meta`: a dict every key of which must be in the file's metadata with that value."""
        blob = torch.load(path, map_location="cpu", weights_only=True)
        cache = cls._from_header(blob, device)
        if expect_meta is not None:
            cache.check_meta(expect_meta)
        if tuple(blob["data"].shape) != tuple(cache.data.shape) or blob["data"].dtype != cache.data.dtype:
            raise ValueError(f"depthg_amd: {path}: the stored table {tuple(blob['data'].shape)} {blob['data'].dtype} is not the "
                             f"{cache._table_text()} its header describes")
        cache.data.copy_(blob["data"])
        cache.filled[:] = blob["filled"].numpy()
        return cache
