"""Segment a folder of images nobody labelled (src/demo_segmentation.py): code and flipped code, both probes at the image's size,
optionally the dense CRF, two 8-bit label PNGs per image.

    python -m depthg_amd.demo --image-dir D --out O --checkpoint F [--res 320] [--batch-size 16] [--crf] [--overlay 0.5] [--cpu]

writes O/linear/<name>.png and O/cluster/<name>.png (mode L: the class id per pixel, 255 where the Hungarian assignment matched no
class) and, with --overlay A, O/linear_rgb/<name>.png and O/cluster_rgb/<name>.png (mode RGB: the PASCAL colours with weight A over the
image).  The images are read with PIL, resized (shorter side to --res, nearest neighbour) and centre-cropped to --res x --res as the
reference's get_transform(res, False, "center") does (src/utils.py:164-182), scaled to [0, 1] and normalised with the ImageNet
constants.  Everything behind that is UnsupervisedSegmenter.segment -> evaluation.segment: one fused HIP launch pair on the GPU;
--cpu runs the reference's torch chain instead (no CRF).

`save_checkpoint(model, path)` / `load_checkpoint(path)` keep {"state_dict", "cfg": vars(cfg), "n_classes", "cluster_assignments"}
with torch.save.  Nothing is ever fetched: a missing file is an error that names it.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .featurizer import DepthGuidance, FrozenBackboneFeaturizer
from .segmenter import UnsupervisedSegmenter

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".ppm", ".tif", ".tiff", ".webp")


def _assignments_of(model):
    """The Hungarian assignment segment() would use, as two lists of ints, or None."""
    for mt in (model.test_cluster_metrics, model.cluster_metrics):
        a = getattr(mt, "assignments", None)
        if a is not None:
            return [[int(v) for v in np.asarray(torch.as_tensor(side)).reshape(-1)] for side in a]
    return None


def save_checkpoint(model: UnsupervisedSegmenter, path: str) -> None:
    """The segmenter's weights, its configuration, its class count and - when a metric's compute() has run - the cluster
    assignment, in one torch.save file of tensors and plain Python values."""
    torch.save({"state_dict": model.state_dict(), "cfg": dict(vars(model.cfg)), "n_classes": int(model.n_classes),
                "cluster_assignments": _assignments_of(model)}, path)


def load_checkpoint(path: str) -> UnsupervisedSegmenter:
    """The segmenter save_checkpoint wrote, on the CPU, in eval mode; its cluster assignment back on test_cluster_metrics."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"depthg_amd.demo: checkpoint {path!r} does not exist (write one with depthg_amd.demo.save_checkpoint; "
                                "nothing is downloaded)")
    ck = torch.load(path, map_location="cpu", weights_only=True)
    missing = [k for k in ("state_dict", "cfg", "n_classes") if k not in ck]
    if missing:
        raise ValueError(f"depthg_amd.demo: {path!r} is not a save_checkpoint file: it lacks {missing}")
    model = UnsupervisedSegmenter(int(ck["n_classes"]), SimpleNamespace(**ck["cfg"]))
    model.load_state_dict(ck["state_dict"])
    a = ck.get("cluster_assignments")
    if a is not None:
        model.test_cluster_metrics.assignments = (np.asarray(a[0], dtype=np.int64), np.asarray(a[1], dtype=np.int64))
    return model.eval()


class TorchHeadFeaturizer(nn.Module):
    """--cpu: a FrozenBackboneFeaturizer's evaluation pass - backbone, then code = cluster1(f) + cluster2(f) (src/modules.py:122-137
    without dropout) - in plain torch, where the fused head has no kernel to run.  Evaluation only."""

    def __init__(self, net: FrozenBackboneFeaturizer):
        super().__init__()
        if isinstance(net, DepthGuidance):
            raise ValueError("depthg_amd.demo: --cpu has no torch route for the depth-guided featurizer (cfg.arch 'dino_depth'); run on the GPU")
        self.net = net

    def forward(self, img):
        if self.training:
            raise RuntimeError("depthg_amd.demo: TorchHeadFeaturizer is an evaluation pass")
        net = self.net
        net.model.eval()
        with torch.no_grad():
            image_feat, _ = net._backbone(img, 1, False)
            if net.proj_type is None:
                return image_feat, image_feat
            cluster1, cluster2 = net._head_modules()
            code = cluster1(image_feat)
            if cluster2 is not None:
                code = code + cluster2(image_feat)
        return image_feat, code


def load_image(path: str, res: int) -> torch.Tensor:
    """One image as the reference's loader hands it over: RGB, shorter side resized to `res` (nearest neighbour), centre crop of
    res x res, [0, 1], normalised.  (3, res, res) fp32."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        w, h = im.size
        if w <= h:
            nw, nh = res, max(res, int(res * h / w))
        else:
            nw, nh = max(res, int(res * w / h)), res
        im = im.resize((nw, nh), Image.NEAREST)
        left, top = int(round((nw - res) / 2.0)), int(round((nh - res) / 2.0))
        im = im.crop((left, top, left + res, top + res))
        x = torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).to(torch.float32) / 255
    mean, std = (torch.tensor(v, dtype=torch.float32).reshape(3, 1, 1) for v in (ops.IMAGENET_MEAN, ops.IMAGENET_STD))
    return (x - mean) / std


def list_images(image_dir: str):
    if not os.path.isdir(image_dir):
        raise FileNotFoundError(f"depthg_amd.demo: image directory {image_dir!r} does not exist")
    names = sorted(n for n in os.listdir(image_dir) if n.lower().endswith(IMAGE_SUFFIXES))
    if not names:
        raise FileNotFoundError(f"depthg_amd.demo: no image ({', '.join(IMAGE_SUFFIXES)}) in {image_dir!r}")
    return names


def run(model: UnsupervisedSegmenter, image_dir: str, out: str, res: int = 320, batch_size: int = 16, crf: bool = False,
        overlay=None, device="cuda:0"):
    """Segment every image of `image_dir` with `model` (already on `device`) and write the PNGs under `out`; returns their names."""
    from PIL import Image
    names = list_images(image_dir)
    kinds = ("linear", "cluster") + (("linear_rgb", "cluster_rgb") if overlay is not None else ())
    for kind in kinds:
        os.makedirs(os.path.join(out, kind), exist_ok=True)
    written = []
    for i in range(0, len(names), batch_size):
        batch = names[i:i + batch_size]
        img = torch.stack([load_image(os.path.join(image_dir, n), res) for n in batch]).to(device)
        seg = model.segment(img, flip=True, run_crf=crf, overlay=overlay)
        for kind in kinds:
            maps = getattr(seg, kind).cpu().numpy()
            for j, n in enumerate(batch):
                new_name = ".".join(n.split(".")[:-1]) + ".png"                    # src/demo_segmentation.py:76
                Image.fromarray(maps[j]).save(os.path.join(out, kind, new_name))  # (H,W) uint8: mode L; (H,W,3): mode RGB
                if kind == "linear":
                    written.append(new_name)
    return written


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m depthg_amd.demo", description=__doc__.split("\n\n")[0])
    ap.add_argument("--image-dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--res", type=int, default=320)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--crf", action="store_true", help="refine both probes with the dense CRF (GPU only)")
    ap.add_argument("--overlay", type=float, default=None, help="also write painted images: the colours' weight in [0, 1] over the image")
    ap.add_argument("--cpu", action="store_true", help="the reference's torch chain on the CPU (no CRF)")
    args = ap.parse_args(argv)
    if args.res < 1 or args.batch_size < 1:
        ap.error("--res and --batch-size must be positive")
    if args.cpu and args.crf:
        ap.error("--crf needs the GPU: the dense CRF has no CPU route here")
    model = load_checkpoint(args.checkpoint)
    if args.res % int(getattr(model.net, "patch_size", 1)):
        ap.error(f"--res must be a multiple of the backbone's patch size ({model.net.patch_size})")
    if args.cpu:
        model.net = TorchHeadFeaturizer(model.net).eval()
        device = "cpu"
    else:
        if not torch.cuda.is_available():
            sys.exit("depthg_amd.demo: no GPU; --cpu runs the reference's torch chain instead")
        device = "cuda:0"
        model = model.to(device)
    written = run(model, args.image_dir, args.out, args.res, args.batch_size, args.crf, args.overlay, device)
    print(f"depthg_amd.demo: {len(written)} image(s) -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
