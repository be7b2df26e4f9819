"""The correlation loss's plan over a sweep of descriptors at feature maps of at most 16384 positions: workspace bytes and the main
kernel's name per descriptor (0 and "" where the descriptor is refused).  tests/golden/corr_plan_sweep.json holds the values of the
commit before feature maps above 16384 positions were served; tests/test_corr_plan_sweep_cpu.py holds the current library to them:
at 16384 positions and below the plan is what it was.  No GPU is needed.

    python scripts/corr_plan_sweep.py [--out tests/golden/corr_plan_sweep.json]      (DEPTHG_TREE: the checkout to record, default this one)
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAPS = [(7, 7, None), (28, 28, None), (32, 32, (8, 8)), (64, 72, (8, 8)), (128, 128, (28, 28)), (7, 7, (56, 56)), (40, 40, None)]


def sweep():
    from depthg_amd import ops
    out = {}
    for (h, w, code_hw), S, C, grad, shared, N, ident in itertools.product(MAPS, [4, 11, 14, 28], [28, 384, 2048], [False, True],
                                                                            [False, True], [0, 5], [False, True]):
        desc = ops.make_desc(4, C, 70, h, w, S, N, pointwise=True, zero_clamp=True, stabalize=False, depth_term=True, need_grad=grad,
                             shared_coords=shared, shifts=(.1, .2, .3, .4), depth_hw=(64, 64), identity_grid=ident, code_hw=code_hw)
        try:
            val = [ops.workspace_bytes(desc), ops.corr_main_kernel_name(desc)]
        except RuntimeError:
            val = [0, ""]
        out[f"{h}x{w} code={code_hw} S={S} C={C} grad={int(grad)} shared={int(shared)} N={N} ident={int(ident)}"] = val
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "corr_plan_sweep.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("DEPTHG_TREE", ROOT))
    table = sweep()
    with open(args.out, "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
    print(f"{len(table)} descriptors, {sum(1 for v in table.values() if v[0])} served -> {args.out}")
