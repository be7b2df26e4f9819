"""cfg.dg_fused_probes in training_step and under GraphedTrainStep, on the 5 x 5 stand-in grid of tests/test_gpu_graph_step.py (12
images, B = 4, a float32 feature cache, deterministic torch algorithms; its helpers are imported, the file is not touched)."""
import pytest
import torch

import probe_step_reference as R
import test_gpu_graph_step as GS
from test_gpu_graph_step import dev  # noqa: F401  (module-scoped fixture, re-used here)

pytestmark = pytest.mark.gpu

MARGIN = 2.0
PROBE_LOGS = ("loss/linear", "loss/cluster", "loss/total")


def test_three_steps_with_the_flag_on_and_off(dev, monkeypatch):
    """From one seed: the probes draw nothing and feed nothing back into the head, so every log but the probes' own - the correlation
    loss's - is the same bits in all steps; the probe losses of step one, where the parameters are still equal, agree within the bound
    of tests/test_gpu_probe_step.py; the nine stepped tensors (cfg.dg_fused_adam) stay finite and close."""
    from depthg_amd import segmenter as S
    monkeypatch.setattr(GS, "STEPS", 3)
    off = GS._run("standin40", dev, False, {}, monkeypatch)
    seen, real = [], S.fused_probe_losses

    def recording(code, label, weight, bias, clusters):
        out = real(code, label, weight, bias, clusters)
        if not seen:
            seen.append(tuple(t.detach().clone() for t in (code, label, weight, bias, clusters)) + (out[0].detach().clone(), out[1].detach().clone()))
        return out
    monkeypatch.setattr(S, "fused_probe_losses", recording)
    on = GS._run("standin40", dev, False, dict(dg_fused_probes=True), monkeypatch)
    assert on[4].fused_probes and not off[4].fused_probes and len(seen) == 1
    for i, ((_, la), (_, lb)) in enumerate(zip(off[0], on[0])):
        assert set(la) == set(lb) and set(PROBE_LOGS) <= set(la)
        others = [k for k in la if k not in PROBE_LOGS]
        assert len(others) >= 4
        for k in others:
            assert torch.equal(GS._bits(la[k]), GS._bits(lb[k])), (i, k)
    # step one: both routes on the same parameters and the same code.  The fused losses, the unfused route's and the float32 torch
    # chain's against the float64 restatement of the step's own operands: each route within MARGIN x the chain's error
    *ops, lin, clu = seen[0]
    t = R.chain(*(x.cpu() for x in ops))
    with torch.no_grad():
        ylin, yclu = R.torch_chain(*ops)
    print(f"step 1: the code's smallest top-two gap {float(R.top_two_gap(ops[0].cpu(), ops[4].cpu()).min()):.3e}")
    for k, name, fused, yard in (("loss/linear", "linear_loss", lin, ylin), ("loss/cluster", "cluster_loss", clu, yclu)):
        floor = R.spacing32(t[name])
        e_fused, e_off, e_yard = (max(abs(float(v) - t[name]), floor) for v in (fused, off[0][0][1][k], yard))
        print(f"step 1 {k}: truth {t[name]!r} fused error {e_fused:.3e} unfused {e_off:.3e} chain {e_yard:.3e}")
        assert float(on[0][0][1][k]) == float(fused)
        assert e_fused <= MARGIN * e_yard and e_off <= MARGIN * e_yard, (k, e_fused, e_off, e_yard)
    assert len(on[1]) == len(off[1]) == 9
    for i, (pa, pb) in enumerate(zip(off[1], on[1])):
        assert bool(torch.isfinite(pb).all())
        # three Adam steps of lr 5e-3 at the most: the two routes' parameters differ by rounding of the gradients only
        assert float((pa - pb).abs().max()) <= 1e-3, (i, float((pa - pb).abs().max()))
    for i in range(6):                                   # the head's six tensors never see the probes
        assert torch.equal(GS._bits(off[1][i]), GS._bits(on[1][i])), i


def test_graphed_steps_with_the_flag_equal_the_eager_steps_with_the_flag(dev, monkeypatch):
    A, G = GS._compare("standin40", dev, dict(dg_fused_probes=True), monkeypatch)
    assert G[2].captures == 1 and G[3] == [False, True, True, True]
    assert G[4].fused_probes and len({float(l) for l, _ in G[0]}) == GS.STEPS


def test_the_probe_reset_step_under_the_flag(dev, monkeypatch):
    """reset_probe_steps = 1: the step with global_step 1 ends by re-drawing both probes and their optimisers; the fused operation reads
    the parameters per call, so the next step trains the new ones.  Graphed and eager agree as in the file this follows."""
    over = dict(dg_fused_probes=True, reset_probe_steps=1)
    A, G = GS._compare("standin40", dev, over, monkeypatch)
    assert G[3] == [False, False, False, True] and G[2].captures == 1
    fresh = GS._run("standin40", dev, False, dict(dg_fused_probes=True), monkeypatch)
    # the reset moved the probes: the losses behind it differ from a run without it, the ones in front do not
    assert float(A[0][1][1]["loss/linear"]) == float(fresh[0][1][1]["loss/linear"])
    assert float(A[0][2][1]["loss/linear"]) != float(fresh[0][2][1]["loss/linear"])
    assert all(bool(torch.isfinite(l)) for l, _ in A[0])
