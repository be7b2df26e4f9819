"""training_step as a driver over stages: six routes of scripts/step_equivalence.py's matrix, at its shapes, two steps each - the exact
log keys, a finite loss, the step count and, where profiles/step_stages.md recorded the parent commit as bit-stable, the same bits
from a second model built from the same seed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import step_equivalence as E  # noqa: E402

pytestmark = pytest.mark.gpu

CORR = {"loss/pos_intra", "loss/pos_inter", "loss/neg_inter", "loss/depth_feat", "cd/pos_intra", "cd/pos_inter", "cd/neg_inter", "cd/depth_feat"}
PROBES = {"loss/linear", "loss/cluster", "loss/total"}
# configuration of the matrix -> (its log keys, whether two runs of the parent commit gave the same bits: profiles/step_stages.md)
CASES = {"pair": (CORR | PROBES, True),
         "pair_deferred": (CORR | PROBES, True),
         "lhp_depth_term": (CORR | PROBES, True),
         "pair_cached": (CORR | PROBES, True),
         "depth_sum_rec": (CORR | PROBES | {"loss/rec"}, False),          # (the depth encoder's backward adds with atomics)
         "aug_gpu_unit": (CORR | PROBES | {"loss/aug_alignment"}, True)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def two_steps(name, dev):
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    over, extras = E.MATRIX[name]
    torch.manual_seed(3)
    seg = UnsupervisedSegmenter(E.N_CLASSES, default_segmenter_cfg(**{**E.BASE, **over})).to(dev).train()
    batch = E.make_batch(dev, seg, extras)
    torch.manual_seed(7)
    out = [seg.training_step(batch, step) for step in range(2)]
    torch.cuda.synchronize()
    return seg, [(loss.clone(), {k: v.clone() for k, v in logs.items()}) for loss, logs in out]


@pytest.mark.parametrize("name", list(CASES))
def test_two_steps(name, dev, monkeypatch):
    # (torch's own convolutions - the stand-in backbone, the linear probe and its backward - with deterministic algorithms)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    keys, bit_stable = CASES[name]
    seg, steps = two_steps(name, dev)
    assert seg.global_step == 2
    for loss, logs in steps:
        assert set(logs) == keys
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v).all()) for v in logs.values())
        assert torch.equal(loss, logs["loss/total"])
    if bit_stable:
        _, again = two_steps(name, dev)
        for (loss, logs), (loss2, logs2) in zip(steps, again):
            assert torch.equal(loss, loss2) and all(torch.equal(logs[k], logs2[k]) for k in keys), name
