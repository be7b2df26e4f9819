"""DeviceEpoch: the batches of a cached epoch chosen on the device.

data.ContrastiveBatches chooses a batch on the host: a slice of the epoch's shuffle, one `torch.randint(...).item()` per sample for its
kNN positive (knn.pick_positive, src/data.py:1079), two index lists checked and uploaded.  With both caches on the card that is all the
host still does for a batch, and it keeps the step from being recorded in a hipGraph.  DeviceEpoch keeps the nearest-neighbour table,
the epoch's order and a three-word generator state on the device; `draw()` is ONE launch (ops.epoch_draw, k_epoch_draw of dg_epoch.hip)
that writes the batch's indices and its positives' into two fixed buffers and advances the state, and `batch()` feeds them to the two
caches' resident-index gathers.  Nothing about a draw is an argument of a launch, so the three launches can be recorded once and
replayed (graph_step.GraphedTrainStep).

Two differences from the reference's loader, both stated in INTEGRATION.md: the positives are a uniform draw from columns
1 .. num_neighbors of the table as the reference's are, but from this class's own Philox stream, not torch.randint's; and the short last
batch of an epoch is DROPPED (steps_per_epoch = n // batch_size): a recorded step has one shape.  The shuffle is the host's -
`torch.randperm(n, generator=...)`, what ContrastiveBatches.__iter__ draws - once per epoch, outside any graph.

On a CPU `device` draw() runs the same arithmetic in numpy (ops.epoch_draw): the statement the kernel is tested against.
"""
import numpy as np
import torch

from . import ops


class DeviceEpoch:
    """DeviceEpoch(nns, batch_size, num_neighbors, device, shuffle=True, generator=None)
        nns                 the table knn.load_nns returns: integer (n_images, K), column 0 the image itself; every entry inside
                            [0, n_images) (checked here, once)
        begin_epoch()       fill `order` in place - torch.randperm(n, generator=generator), or arange without `shuffle` - and zero the
                            cursor: the only host work of an epoch, outside any graph
        steps_per_epoch     n_images // batch_size: the short last batch is dropped
        draw()              one launch: (ind, ind_pos), the two FIXED int64 (batch_size,) buffers, rewritten by every draw
        batch(sample_cache, feature_cache)   draw(), then the caches' gathers from the resident indices: the dictionary
                            data.ContrastiveBatches.batch_of returns - same keys, shapes and dtypes - but for `ind` / `ind_pos`, which stay
                            on the device
        state               int64 {seed, draws, cursor} on the device; the seed comes from torch's CPU generator (ops.new_perm_state)
        drawn               batches drawn since begin_epoch (host count: draw() refuses to run past the epoch's end)
    The caches' "row was never put" checks cannot run per batch (the indices are on the device): `batch` asks each cache ONCE, the
    first time it sees it, that every row is filled, that it holds n_images rows and lives on this device."""

    def __init__(self, nns, batch_size, num_neighbors, device, shuffle=True, generator=None):
        table = torch.as_tensor(np.ascontiguousarray(nns) if isinstance(nns, np.ndarray) else nns)
        if table.dim() != 2 or table.is_floating_point() or table.dtype == torch.bool or table.shape[0] < 1:
            raise ValueError(f"depthg_amd: DeviceEpoch wants the nearest-neighbour table as an integer (n_images, K) array, got "
                             f"{tuple(table.shape)} {table.dtype}")
        table = table.to(torch.int64)
        self.n_images, self.K = int(table.shape[0]), int(table.shape[1])
        self.batch_size, self.num_neighbors = int(batch_size), int(num_neighbors)
        if self.batch_size < 1 or self.batch_size > ops.EPOCH_DRAW_MAX_B:
            raise ValueError(f"depthg_amd: DeviceEpoch: batch_size={batch_size} outside [1, {ops.EPOCH_DRAW_MAX_B}] (one block draws the batch)")
        if self.batch_size > self.n_images:
            raise ValueError(f"depthg_amd: DeviceEpoch: batch_size={batch_size} above the {self.n_images} images of the table: the short last "
                             "batch is dropped, so such an epoch has no batch")
        if self.num_neighbors < 1 or self.num_neighbors >= self.K:
            raise ValueError(f"depthg_amd: DeviceEpoch: num_neighbors={num_neighbors} outside [1, {self.K - 1}] of a table with {self.K} "
                             "columns (column 0 is the image itself)")
        if int(table.min()) < 0 or int(table.max()) >= self.n_images:
            raise IndexError(f"depthg_amd: DeviceEpoch: the nearest-neighbour table names an image outside [0, {self.n_images})")
        self.shuffle, self.generator = bool(shuffle), generator
        self.nns = table.contiguous().to(torch.device(device))
        self.device = self.nns.device                            # ("cuda" has become "cuda:0": what the caches' tensors say)
        self.order = torch.arange(self.n_images, dtype=torch.int64, device=self.device)
        self.state = ops.new_perm_state(self.device)
        self.ind = torch.zeros(self.batch_size, dtype=torch.int64, device=self.device)
        self.ind_pos = torch.zeros(self.batch_size, dtype=torch.int64, device=self.device)
        self.steps_per_epoch = self.n_images // self.batch_size
        self.drawn = self.steps_per_epoch          # (no epoch begun yet)
        self._checked = []

    def __len__(self):
        return self.steps_per_epoch

    def begin_epoch(self):
        """The epoch's order into the fixed buffer, the cursor to zero (`draws` goes on: every epoch draws other positives)."""
        if self.shuffle:
            self.order.copy_(torch.randperm(self.n_images, generator=self.generator))
        self.state[2:3].zero_()
        self.drawn = 0

    def _count(self):
        if self.drawn >= self.steps_per_epoch:
            raise RuntimeError(f"depthg_amd: DeviceEpoch: all {self.steps_per_epoch} batches of this epoch are drawn (or none was begun): "
                               "call begin_epoch()")
        self.drawn += 1

    def draw(self):
        self._count()
        return ops.epoch_draw(self.state, self.order, self.nns, self.batch_size, self.num_neighbors, self.ind, self.ind_pos)

    def replayed(self):
        """A recorded draw() was replayed: the host's count of the epoch's batches follows the device's cursor."""
        self._count()

    def _check_cache(self, cache, role):
        if any(c is cache for c in self._checked):
            return
        where = getattr(getattr(cache, "data", None), "device", cache.device)
        if cache.n_images != self.n_images or where != self.device:
            raise ValueError(f"depthg_amd: DeviceEpoch: the {role} holds {cache.n_images} images on {where}, the epoch draws from "
                             f"{self.n_images} on {self.device}")
        if not bool(cache.filled.all()):
            raise ValueError(f"depthg_amd: DeviceEpoch: row {int(np.flatnonzero(~cache.filled)[0])} of the {role} was never put: an epoch "
                             "drawn on the device may name any row, fill the whole cache first (data.build_sample_cache / build_feature_cache)")
        self._checked.append(cache)

    def batch(self, sample_cache, feature_cache=None, label_dims=3, return_depth=None):
        """The batch dictionary of the next draw.  label_dims: the dataset's (4: label and mask carry a channel axis); return_depth:
        whether the batch carries depth / depth_pos (None: when the sample cache has a depth plane)."""
        self._check_cache(sample_cache, "sample cache")
        if feature_cache is not None:
            self._check_cache(feature_cache, "feature cache")
        if self.device.type != "cuda":
            raise RuntimeError("depthg_amd: DeviceEpoch.batch gathers with the caches' kernels from indices on the GPU; there is no CPU path")
        B = self.batch_size
        ind, ind_pos = self.draw()
        sc = sample_cache
        out = ops.sample_cache_gather(sc.data, sc.has_labels, sc.with_depth, ind, ind_pos, label_offset=sc.label_offset, fill=sc.fill,
                                      mask_rule=sc.mask_rule, mean=ops.IMAGENET_MEAN, std=ops.IMAGENET_STD)
        img, label, mask, depth = out["img"], out["label"], out["mask"], out.get("depth")
        if label_dims == 4:
            label = label.unsqueeze(1)
        if label_dims == 4 or sc.mask_rule == ops.BATCH_MASK_BOOL_IGNORED:
            mask = mask.unsqueeze(1)
        with_depth = sc.with_depth if return_depth is None else bool(return_depth)
        if with_depth and depth is None:
            raise ValueError("depthg_amd: DeviceEpoch.batch: depth was asked for but the sample cache has no depth plane")
        batch = {"ind": ind, "img": img[:B], "label": label[:B], "mask": mask[:B]}
        if with_depth:
            batch["depth"] = depth[:B].unsqueeze(1)
        batch.update({"img_pos": img[B:], "ind_pos": ind_pos, "label_pos": label[B:], "mask_pos": mask[B:]})
        if with_depth:
            batch["depth_pos"] = depth[B:].unsqueeze(1)
        if feature_cache is not None:
            feats = ops.feature_cache_gather(feature_cache.data, ind, ind_pos).reshape((2 * B,) + feature_cache.shape)
            batch["image_feat"], batch["image_feat_pos"] = feats[:B], feats[B:]
        return batch
