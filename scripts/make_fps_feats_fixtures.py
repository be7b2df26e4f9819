"""Generate tests/golden/fps_feats_*.npz on the CPU: margin inputs and the `sample_inds` the reference's own fps_depth_feats
(src/modules.py:1124-1180) returns on them.  The function is imported from a reference checkout at run time (the import recipe of
tests/golden/make_fixtures.py); only arrays are written.

    python scripts/make_fps_feats_fixtures.py [--reference DIR] [--search]

Without --search the seeds recorded in tests/fps_feats_reference.py CASES are used and re-checked.  With --search every case takes the
first seed from 0 up whose float64 margin (fps_feats_reference.MARGIN) holds, and the accepted seeds are printed for CASES.
Per case the file keeps the images' seeds, shape, checksum of the drawn inputs and `sample_inds` (B, S*S); the inputs themselves when they are a
few KB, else the tests re-draw them from the seed and hold them to the checksum."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import fps_feats_reference as R  # noqa: E402
from oracle import depthg_oracle as O  # noqa: E402

KEEP_INPUT_BYTES = 16 * 1024


def checksum(depth, feats):
    return np.asarray([depth.astype(np.float64).sum(), np.abs(depth.astype(np.float64)).sum(), feats.astype(np.float64).sum(),
                       np.abs(feats.astype(np.float64)).sum()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DEPTHG_REFERENCE"), help="the reference checkout (default: make_fixtures.REF)")
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--max-seeds", type=int, default=20000)
    args = ap.parse_args()
    import make_fixtures as MF
    if args.reference:
        MF.REF = args.reference
    M, _ = MF.import_reference()
    accepted = {}
    for name, (seeds, C, h, w, H, W, S) in R.CASES.items():
        flat = name.startswith("flat_depth")
        found = []
        for b, seed in enumerate(seeds):          # every image of a case is searched on its own
            tries = range(args.max_seeds) if args.search or seed is None else [seed]
            for s in tries:
                if s in found:
                    continue
                depth, feats = R.margin_inputs((s,), C, h, w, H, W, S, flat)
                _, inds, margin = R.sample(depth, feats, S, np.float64, want_margin=True)
                # (the flat-depth case is there to show the feature term deciding: its selection must leave the depth-only sampler's)
                if margin >= R.MARGIN and not (flat and np.array_equal(
                        np.sort(inds), np.sort(O.farthest_point_sampling_depth((h, w), torch.from_numpy(depth), S, return_inds=True)[1]))):
                    break
            else:
                raise SystemExit(f"{name}: image {b}: no seed below {args.max_seeds} holds the margin")
            found.append(s)
        accepted[name] = tuple(found)
        depth, feats = R.margin_inputs(found, C, h, w, H, W, S, flat)
        B = len(found)
        _, inds64, margin = R.sample(depth, feats, S, np.float64, want_margin=True)
        # the reference's own function on the reference's own operands (:1003, :1016-1017)
        t, d = torch.from_numpy(feats), torch.from_numpy(depth)
        pooled = torch.nn.functional.adaptive_avg_pool2d(d, t.shape[-2:])
        ref = []
        for i in range(B):
            cloud = M.depth2points(pooled[i].squeeze(), fov=90).permute(1, 2, 0).reshape(-1, 3)
            rows = t[i].permute(1, 2, 0).reshape(-1, t.shape[1])
            ref.append(np.asarray(M.fps_depth_feats(cloud, rows, S * S)[1], np.int64))
        ref = np.stack(ref)
        _, inds32 = R.sample(depth, feats, S, np.float32)
        assert np.array_equal(ref, inds64) and np.array_equal(ref, inds32), f"{name}: the restatement leaves the reference at seeds {found}"
        out = dict(seeds=np.asarray(found, np.int64), shape=np.asarray([B, C, h, w, H, W, S], np.int64), input_checksum=checksum(depth, feats),
                   sample_inds=ref, margin=np.float64(margin))
        if depth.nbytes + feats.nbytes <= KEEP_INPUT_BYTES:
            out.update(depth=depth, feats=feats)
        path = os.path.join(ROOT, "tests", "golden", f"fps_feats_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: seeds {found}, margin {margin:.3e}, {os.path.getsize(path)} bytes")
    print("CASES seeds:", accepted)


if __name__ == "__main__":
    main()
