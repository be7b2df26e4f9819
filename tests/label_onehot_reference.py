"""The reference's one-hot label signal (src/train_segmentation.py:219-225; one_hot_feats, src/utils.py:64-65) restated on torch, and the
label maps the cfg.use_true_labels tests share."""
import torch
import torch.nn.functional as F


def one_hot_signal(label, n_classes):
    """one_hot_feats(label + 1, n_classes + 1): int64 (B,H,W) with values in [-1, n_classes - 1] -> fp32 (B, n_classes + 1, H, W)."""
    return F.one_hot(label + 1, n_classes + 1).permute(0, 3, 1, 2).to(torch.float32)


def random_labels(seed, B, n_classes, H, W):
    """int64 (B,H,W), uniform over [-1, n_classes - 1], with both ends of the range present wherever the map has two pixels."""
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(-1, n_classes, (B, H, W), generator=g)
    flat = label.view(-1)
    flat[0] = n_classes - 1
    if flat.numel() > 1:
        flat[-1] = -1
    return label


# (B, K, H, W) of the issue's kernel cases, K = n_classes + 1 channels: a ragged map (W % 4 != 0: one pixel per lane), one pixel, a map of
# whole 16-byte vectors in one block per image, the same with a block that ends inside the map, the widest signal
ONEHOT_SHAPES = [(2, 4, 5, 7), (1, 2, 1, 1), (3, 28, 32, 32), (2, 28, 20, 68), (1, 256, 8, 12)]
