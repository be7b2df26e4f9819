"""d loss / d image_feat of the projection head (ProjectionHead(..., input_grad=True) -> dg_head_backward_input, k_head_dx)
against float64 autograd of oracle.head_oracle.head_forward, on every case of tests/head_margin_inputs.py - dh_route FUSED and TILES,
step-major and row-major d hidden, the linear head, the pair form, C = 256 / 352 / 384 / 768, D = 70 / 96 / 100, P = 225 - and two
small cases of tests/head_input_grad_reference.py (an eval-mode head without keep masks; a pair in which only the second pass
requires grad).  The inputs flip no ReLU mask, so the kernel must reproduce the oracle to the accuracy of its operand formats:
every figure of head_margin_inputs.tensor_errors(..., "code") within FACTOR x the yardstick's (the float64 restatement with each
operand rounded to bf16 where the kernel rounds it) and every L2 below CAP_L2.  Each case asserts its routes through ops.head_plan
first and prints kernel figure, yardstick and ratio before asserting (-s shows them; profiles/head_input_grad_parity.md holds the
table of an MI355X run).  Per case also: the six parameter gradients bit-identical with input_grad on and off, two calls with
identical dx bits, channels dropped by both masks exactly zero, everything finite with poisoned buffers (ops.POISON)."""
import pytest
import torch

import head_input_grad_reference as R
import head_margin_inputs as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def make_head(case, inp, dev, train=True):
    from depthg_amd.head import ProjectionHead
    head = ProjectionHead(case.C, case.D, case.proj).to(dev).train(train)
    given = (inp.w1, inp.b1) + ((inp.w2a, inp.b2a, inp.w2b, inp.b2b) if case.proj == "nonlinear" else ())
    with torch.no_grad():
        for (name, prm), t, want_name in zip(head.named_parameters(), given, H.PARAMS):
            assert name == want_name
            prm.copy_(t.reshape(prm.shape))
    return head


def run_case(case, inp, dev, input_grad, need=(True, True)):
    """One forward + backward -> (dx per pass (None where the pass does not ask), {parameter name: gradient})."""
    head = make_head(case, inp, dev, train=inp.keeps is not None)
    T = lambda t: t.to(dev)
    keeps = None if inp.keeps is None else tuple(T(k) for k in inp.keeps)
    feat, up = T(inp.feat), T(inp.up)
    if case.pair:
        B = case.B
        fa, fb = (feat[:B].clone().requires_grad_(input_grad and need[0]), feat[B:].clone().requires_grad_(input_grad and need[1]))
        (c1, _), (c2, _) = head.forward_pair(fa, fb, True, keeps, input_grad=input_grad)
        ((c1 * up[:B]).sum() + (c2 * up[B:]).sum()).backward()
        dx = (fa.grad, fb.grad)
    else:
        fa = feat.clone().requires_grad_(input_grad)
        code, _ = head(fa, True, keeps, input_grad=input_grad)
        (code * up).sum().backward()
        dx = (fa.grad,)
    torch.cuda.synchronize()
    return dx, {name: prm.grad for name, prm in head.named_parameters()}


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_input_gradient_within_factor_of_operand_yardstick(case, dev, monkeypatch):
    from depthg_amd import ops
    torch.set_num_threads(16)
    plan = H.check_plan(case)                                   # 1. the routes this case is about, from the library's own plan
    print(f"{case.id} {plan}")
    ref = R.case_reference(case.id)
    inp = ref.inp
    second_only = case.id == R.SMALL_PAIR.id
    need = (False, True) if second_only else (True, True)
    monkeypatch.setattr(ops, "POISON", True)                    # (every buffer the layer hands out starts as 0xFF bytes: NaN)
    dx, grads_on = run_case(case, inp, dev, True, need)
    if second_only:
        assert dx[0] is None and dx[1] is not None              # (a pass that does not ask gets None)
        got, images = dx[1], slice(case.B, 2 * case.B)
    else:
        got, images = torch.cat(dx), slice(None)
    assert bool(torch.isfinite(got).all())
    lines, bad = R.compare(case, got, images)                   # 2. print every figure, then assert
    for line in lines:
        print(line)
    assert not bad, bad
    # 3. the parameter gradients do not depend on the keyword; two calls give the same dx bits
    dx_again, grads_again = run_case(case, inp, dev, True, need)
    _, grads_off = run_case(case, inp, dev, False)
    assert set(grads_on) == set(grads_off) == set(H.PARAMS[:6 if case.proj == "nonlinear" else 2])
    for name in grads_on:
        assert torch.equal(grads_on[name], grads_off[name]), name
        assert torch.equal(grads_on[name], grads_again[name]), name
        assert bool(torch.isfinite(grads_on[name]).all()), name
    for a, b in zip(dx, dx_again):
        assert (a is None and b is None) or torch.equal(a, b)
    # 4. a channel dropped by both masks carries exactly nothing
    if inp.keeps is not None:
        k2 = inp.keeps[1] if case.proj == "nonlinear" else torch.zeros_like(inp.keeps[0])
        dropped = ((inp.keeps[0] == 0) & (k2 == 0))[images].to(dev)
        assert int(dropped.sum()) > 0 or case.C < 128
        assert bool((got[dropped] == 0).all())


def test_default_still_refuses_features_that_require_grad(dev):
    from depthg_amd.head import ProjectionHead
    head = ProjectionHead(64, 16).to(dev).train()
    feat = torch.randn(2, 64, 3, 3, device=dev)
    with pytest.raises(RuntimeError, match="require grad"):
        head(feat.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="require grad"):
        head.forward_pair(feat, feat.clone().requires_grad_())
    code, _ = head(feat.clone().requires_grad_(), input_grad=True)
    assert code.requires_grad
