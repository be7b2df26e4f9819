"""The correlation loss's code gradient (d/d code, d/d code_pos) of the DEFAULT kernels, per position row, channel and element,
on inputs that cannot flip a clamp mask (tests/margin_inputs.py; tests/test_margin_inputs_cpu.py pins the inputs on the CPU).

The other parity tests bound the gradient of the default kernels by 2-4 % of its L2 norm on grids above 160 positions: that is
what the mask flips of the fp16 cd chain cost on random code maps (header of tests/test_gpu_parity.py), and one wrong position row, a
ragged tile's missing row or a pair-set factor 2 % off hides under it.  Here no cd lies within 0.05 of a clamp bound, so the same
kernels - k_corr2<.., XM = false, ..> with and without the fold, k_gs, the dense scatter / k_combine_out with fp16 gradient tiles,
the taps scatter, k_corr_main where the exact-mask flag is refused - must reproduce a float64 oracle to the accuracy of their
operand formats: every figure of margin_inputs.grad_errors within FACTOR[family] x the operand yardstick's, under the caps CAP_*.
Every case asserts its route with the library's own predicates first and prints kernel figure, yardstick and ratio before asserting
(-s shows them; profiles/grad_margin.md holds the table of an MI355X run, and three seeded arithmetic defects that these cases
catch and test_dense_grid_shapes does not)."""
import pytest
import torch

import margin_inputs as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def run_case(case, dev):
    """One case on the GPU -> (cfg, loss module, out tuple, total, d/d code, d/d code_pos)."""
    from depthg_amd import ContrastiveCorrelationLoss
    from oracle import depthg_oracle as O
    cfg, inp, _ = M.case_reference(case.id)
    f, fp, c, cp, d, c1, c2, perms = inp
    T = lambda t: t.to(dev)
    cg, cpg = T(c).requires_grad_(True), T(cp).requires_grad_(True)
    ident = case.coords == "identity"
    loss = ContrastiveCorrelationLoss(cfg)
    out = loss.forward_with(T(f), T(fp), cg, cpg, T(d), T(c1), T(c2), [T(p) for p in perms], shared_coords=ident, identity_grid=ident)
    total = O.total_loss(cfg, out)
    total.backward()
    torch.cuda.synchronize()
    return cfg, loss, out, total, cg.grad, cpg.grad


def measure_case(case, dev):
    """Everything the test asserts on, as numbers: route, loss-mean errors, the four figures per tensor with their yardsticks."""
    from depthg_amd import ops
    torch.set_num_threads(16)
    cfg, inp, ref = M.case_reference(case.id)
    yard = M.operand_yardstick(cfg, *inp, ref=ref)
    _, loss, out, total, g_code, g_code_pos = run_case(case, dev)
    desc = loss.last_call[0]
    res = {"id": case.id, "family": case.family, "kernel": ops.corr_main_kernel_name(desc), "folded": ops.corr_intra_folded(desc),
           "means": {}, "finite": bool(torch.isfinite(g_code).all()) and bool(torch.isfinite(g_code_pos).all())}
    for name, got, want in (("intra", out[0], ref[0][0]), ("inter", out[2], ref[0][2]), ("neg", out[4].mean(), ref[0][4].mean()),
                            ("depth", out[6], ref[0][6]), ("total", total, ref[1])):
        res["means"][name] = (float(got.detach()), float(want))
    for name, got, want in (("code", g_code, ref[2]), ("code_pos", g_code_pos, ref[3])):
        res[name] = {"kernel": M.grad_errors(got, want), "yardstick": yard[name], "where": M.worst_locations(got, want)}
    return res


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_gradient_within_factor_of_operand_yardstick(case, dev):
    res = measure_case(case, dev)
    # 1. the route this case is about
    assert res["kernel"] == case.kernel, res["kernel"]
    assert res["folded"] == (case.kernel == "k_corr2" and case.pointwise)
    # 2. loss means and the total, within the bounds these routes already carry
    rtol, atol = (2e-5, 0.0) if (case.coords == "identity" and case.hw % 8 == 0) else (1e-3, 1e-5)
    for name, (got, want) in res["means"].items():
        print(f"{case.id} {name}: got {got:.9e} want {want:.9e} rel {abs(got - want) / abs(want):.2e}")
    # 3. the gradients: print, then assert
    bad = []
    for name in ("code", "code_pos"):
        r = res[name]
        for fig, k, y in zip(M.FIGURES, r["kernel"], r["yardstick"]):
            cap = {"l2": M.CAP_L2[name], "row": M.CAP_ROW, "channel": M.CAP_CHANNEL, "elem": float("inf")}[fig]
            factor = getattr(M.FACTOR[case.family], fig)
            print(f"{case.id} d/d {name} {fig}: kernel {k:.3e} yardstick {y:.3e} ratio {k / y:.2f} (factor {factor}, cap {cap:.0e})"
                  + (f" at {r['where'][fig]}" if fig in r["where"] else ""))
            if not (k <= factor * y and k <= cap):
                bad.append((name, fig, k, y, factor, cap))
    for name, (got, want) in res["means"].items():
        assert abs(got - want) <= rtol * abs(want) + atol, (name, got, want)
    assert not bad, bad
    assert res["finite"]
