"""The projection head's backward where its persistent kernels loop, per row, column and element, on inputs that cannot flip a ReLU
mask (tests/head_margin_inputs.py; tests/test_head_margin_inputs_cpu.py pins the inputs, the yardstick and the plan on the CPU).

tests/test_gpu_head.py compares the head with an oracle at B <= 4: every k_head_dh2 block processes one tile, every split of
k_head_wgrad3 covers one or two steps, and a parameter gradient may be 2e-2 (6e-2 behind the ReLU) of its L2 norm off.  The cases
here are the smallest on which a k_head_dh2 block walks three tiles (the second LDS image, the prefetch, d W2b accumulated over
tiles), the DMA ring of k_head_wgrad3 wraps and its splits cross image boundaries, and on which the plan's other route
combinations run (k_head_dh2 in front of k_head_wgrad2, k_head_wgrad3 on a row-major d hidden, the grouped linear head with the
768-block split target, ViT-B width, an odd map).  No pre-activation lies within four times its rounding error of zero, so the
kernels must reproduce a float64 oracle to the accuracy of their operand formats: every figure of
head_margin_inputs.tensor_errors within FACTOR x the operand yardstick's and every L2 figure below 2e-2, for the six (two) parameter
gradients and for code.  Every case asserts its route with the library's own plan first and prints kernel figure, yardstick, ratio
and location before asserting (-s shows them; profiles/head_grad_margin.md holds the table of an MI355X run and three seeded
arithmetic defects that these cases catch and tests/test_gpu_head.py does not)."""
import pytest
import torch

import head_margin_inputs as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def run_case(case, dev):
    """One case on the GPU -> ({tensor name: value}, the returned feats per pass)."""
    from depthg_amd.head import ProjectionHead
    inp = H.case_reference(case.id).inp
    head = ProjectionHead(case.C, case.D, case.proj).to(dev).train()
    given = (inp.w1, inp.b1) + ((inp.w2a, inp.b2a, inp.w2b, inp.b2b) if case.proj == "nonlinear" else ())
    with torch.no_grad():
        for (name, prm), t, want_name in zip(head.named_parameters(), given, H.PARAMS):
            assert name == want_name
            prm.copy_(t.reshape(prm.shape))
    T = lambda t: t.to(dev)
    keeps, feat, up = tuple(T(k) for k in inp.keeps), T(inp.feat), T(inp.up)
    if case.pair:
        B = case.B
        (c1, f1), (c2, f2) = head.forward_pair(feat[:B].contiguous(), feat[B:].contiguous(), True, keeps)
        ((c1 * up[:B]).sum() + (c2 * up[B:]).sum()).backward()
        code, feats = torch.cat([c1, c2]), torch.cat([f1, f2])
    else:
        code, feats = head(feat, True, keeps)
        (code * up).sum().backward()
    torch.cuda.synchronize()
    got = {name: prm.grad for name, prm in head.named_parameters()}
    got["code"] = code.detach()
    return got, feats


@pytest.mark.parametrize("case", H.CASES, ids=[c.id for c in H.CASES])
def test_head_gradients_within_factor_of_operand_yardstick(case, dev):
    torch.set_num_threads(16)
    plan = H.check_plan(case)                                   # 1. the route this case is about
    print(f"{case.id} {plan}")
    got, feats = run_case(case, dev)
    lines, bad = H.compare(case, got)                           # 2. print every figure, then assert
    for line in lines:
        print(line)
    assert not bad, bad
    inp = H.case_reference(case.id).inp
    want_feats = inp.feat * (inp.keeps[2] * (1.0 / (1.0 - H.P_DROP)))[:, :, None, None]
    assert torch.allclose(feats.cpu(), want_feats, rtol=1e-6, atol=0)
    assert all(bool(torch.isfinite(t).all()) for t in got.values()) and bool(torch.isfinite(feats).all())
