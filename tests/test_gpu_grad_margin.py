"""The correlation loss's fused total (`loss.total`, DG_OUT_TOTAL) and its code gradient (d/d code, d/d code_pos) of the DEFAULT kernels,
per position row, channel and element, on inputs that cannot flip a clamp mask (tests/margin_inputs.py; tests/test_margin_inputs_cpu.py
pins the inputs on the CPU).

The other parity tests bound the gradient of the default kernels by 2-4 % of its L2 norm on grids above 160 positions: that is
what the mask flips of the fp16 cd chain cost on random code maps (header of tests/test_gpu_parity.py), and one wrong position row, a
ragged tile's missing row or a pair-set factor 2 % off hides under it.  Here no cd lies within 0.05 of a clamp bound, so the same
kernels - k_corr2<.., XM = false, ..> with and without the fold, k_gs, the dense scatter / k_combine_out with fp16 gradient tiles,
the taps scatter, k_corr_main where the exact-mask flag is refused, the fused small-grid kernel, the channel chunks of maps wider than
768 on the dense and on sampled grids, code maps of another size, the line grid, one shared sample grid - must reproduce a float64
oracle to the accuracy of their operand formats: every figure of margin_inputs.grad_errors within FACTOR[family] x the operand
yardstick's, under the caps CAP_*.
The backward starts at `loss.total`, the in-kernel weighted total that training.fused_correspondence_total and the segmenter train on,
not at the oracle's arithmetic on the returned tuple: `loss.total` is held to the float64 oracle's total and to O.total_loss(cfg, out) of
the same forward, so the weights, the shifts, correspondence_weight and the lhp balance of every launch set are part of what is checked
(the weights cases: margin_inputs.WEIGHTS).
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
    """One case on the GPU -> (cfg, loss module, out tuple, total, d/d code, d/d code_pos, tuple total, descriptors of the launch sets).
    total is `loss.total`, and the backward starts there; the tuple total is O.total_loss(cfg, out) of the same forward."""
    from depthg_amd import ContrastiveCorrelationLoss
    from oracle import depthg_oracle as O
    cfg, inp, _ = M.case_reference(case.id)
    f, fp, c, cp, d, c1, c2, perms = inp
    T = lambda t: t.to(dev)
    cg, cpg = T(c).requires_grad_(True), T(cp).requires_grad_(True)
    ident = case.coords == "identity"
    loss = ContrastiveCorrelationLoss(cfg)
    descs, run_chunk = [], loss._run_chunk

    def recording(*a, **kw):                 # every launch set the call runs (one per channel chunk), in order
        res = run_chunk(*a, **kw)
        descs.append(res[2])
        return res
    loss.__dict__["_run_chunk"] = recording
    out = loss.forward_with(T(f), T(fp), cg, cpg, T(d), T(c1), T(c2), [T(p) for p in perms], shared_coords=ident or case.coords == "shared",
                            identity_grid=ident)
    total = loss.total
    tuple_total = O.total_loss(cfg, out).detach()
    total.backward()
    torch.cuda.synchronize()
    return cfg, loss, out, total.detach(), cg.grad, cpg.grad, tuple_total, descs


def route_of(case, loss, descs):
    """What the library reports about the launch sets of a call, and what the case expects of them, as two dicts."""
    from depthg_amd import _lib, ops
    first = descs[0]
    flag = lambda d, name: bool(d.flags & getattr(_lib, name))
    hc = case.code_hw if case.code_hw not in (None, case.hw) else 0
    got = {"kernel": ops.corr_main_kernel_name(first), "folded": ops.corr_intra_folded(first), "chunks": len(descs),
           "chunk_channels": [int(d.C) for d in descs], "last_call_is_first_chunk": loss.last_call[0] is first,
           "identity": flag(first, "DG_IDENTITY_GRID"), "shared": flag(first, "DG_SHARED_COORDS"), "line": flag(first, "DG_LINE_GRID"),
           "depth": flag(first, "DG_DEPTH_TERM"), "exact": flag(first, "DG_EXACT_MASKS"), "unit": flag(first, "DG_FEATS_UNIT"),
           "code_hw": (int(first.code_h), int(first.code_w)),
           # launch sets after the first: no depth term, zero shifts, no depth weight, the first one's kernel
           "later": [(flag(d, "DG_DEPTH_TERM"), (d.shift_intra, d.shift_inter, d.shift_neg, d.shift_depth), d.w_depth,
                      ops.corr_main_kernel_name(d)) for d in descs[1:]]}
    ident = case.coords == "identity"
    chunk_c = loss._chunk_channels(case.C) if case.chunks > 1 else case.C
    want = {"kernel": case.kernel, "folded": case.kernel == "k_corr2" and case.pointwise, "chunks": case.chunks,
            "chunk_channels": [min(chunk_c, case.C - k * chunk_c) for k in range(case.chunks)], "last_call_is_first_chunk": True,
            "identity": ident, "shared": ident or case.coords == "shared", "line": case.coords == "line", "depth": case.depth_term,
            "exact": bool(case.over.get("dg_exact_masks", False)), "unit": ident and case.chunks > 1, "code_hw": (hc, hc),
            "later": [(False, (0.0, 0.0, 0.0, 0.0), 0.0, case.kernel)] * (case.chunks - 1)}
    return got, want


def measure_case(case, dev):
    """Everything the test asserts on, as numbers: route, loss-mean errors, the four figures per tensor with their yardsticks."""
    torch.set_num_threads(16)
    cfg, inp, ref = M.case_reference(case.id)
    yard = M.operand_yardstick(cfg, *inp, ref=ref)
    _, loss, out, total, g_code, g_code_pos, tuple_total, descs = run_case(case, dev)
    assert len(out) == len(ref[0]) == (8 if case.depth_term else 6)
    res = {"id": case.id, "family": case.family, "route": route_of(case, loss, descs), "means": {},
           "tuple_total": (float(total), float(tuple_total)),
           "finite": bool(torch.isfinite(g_code).all()) and bool(torch.isfinite(g_code_pos).all())}
    # (a wide map: out[0], out[2], out[4] are the sums over the chunks, out[6] is the first chunk's)
    means = [("intra", out[0], ref[0][0]), ("inter", out[2], ref[0][2]), ("neg", out[4].mean(), ref[0][4].mean())]
    if case.depth_term:
        means.append(("depth", out[6], ref[0][6]))
    for name, got, want in means + [("total", total, ref[1])]:
        res["means"][name] = (float(got.detach()), float(want))
    for name, got, want in (("code", g_code, ref[2]), ("code_pos", g_code_pos, ref[3])):
        res[name] = {"kernel": M.grad_errors(got, want), "yardstick": yard[name], "where": M.worst_locations(got, want)}
    return res


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_gradient_within_factor_of_operand_yardstick(case, dev):
    res = measure_case(case, dev)
    # 1. the route this case is about
    got, want = res["route"]
    print(f"{case.id} route: {got}")
    assert got == want
    # 2. loss means and the fused total, within the bounds these routes already carry; the fused total against the tuple's
    rtol, atol = (2e-5, 0.0) if (case.coords == "identity" and case.hw % 8 == 0) else (1e-3, 1e-5)
    for name, (got, want) in res["means"].items():
        print(f"{case.id} {name}: got {got:.9e} want {want:.9e} rel {abs(got - want) / abs(want):.2e}")
    fused, from_tuple = res["tuple_total"]
    print(f"{case.id} loss.total {fused:.9e} O.total_loss(cfg, out) {from_tuple:.9e} rel {abs(fused - from_tuple) / abs(from_tuple):.2e}")
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
    assert fused == pytest.approx(from_tuple, rel=1e-5, abs=1e-9)
    assert not bad, bad
    assert res["finite"]
