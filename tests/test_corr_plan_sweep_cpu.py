"""At feature maps of 16384 positions and below the correlation loss's plan is what it was before larger maps were served: workspace
bytes and main kernel of 1344 descriptors against the values recorded from the preceding commit's library
(tests/golden/corr_plan_sweep.json, scripts/corr_plan_sweep.py)."""
import json
import os
import sys

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_plan_is_unchanged_at_and_below_the_old_limit():
    from corr_plan_sweep import sweep
    want = json.load(open(os.path.join(GOLDEN, "corr_plan_sweep.json")))
    got = sweep()
    assert len(want) == len(got) == 1344 and sum(1 for v in want.values() if v[0]) > 500
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, f"{len(diff)} descriptors changed, e.g. {next(iter(diff.items()))}"
