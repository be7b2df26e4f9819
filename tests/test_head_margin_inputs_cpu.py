"""CPU side of the per-row check of the projection head's backward (tests/head_margin_inputs.py): on the inputs of every case of
tests/test_gpu_head_margin.py no rounding of the operands can flip a ReLU mask while the mask still varies inside every plane, the
operand yardstick is a small non-zero number, the library's plan puts every case on the path it is about, and the error figures
measure what they say.  No GPU: float64 arithmetic and the host-side plan only."""
import math

import pytest
import torch

import head_margin_inputs as H

IDS = [c.id for c in H.CASES]
NONLINEAR = [c.id for c in H.CASES if c.proj == "nonlinear"]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(16)


@pytest.mark.parametrize("case_id", NONLINEAR)
def test_case_inputs_cannot_flip_a_mask(case_id):
    """A condition on the inputs (the seeds of the table are chosen for it)."""
    m = H.case_reference(case_id).masks
    print(case_id, m)
    assert m["flips"] == 0, f"{m['flips']} masks flip under the operand rounding (min |pre| {m['min_abs']:.4f}, deviation {m['deviation']:.4f})"
    assert m["min_abs"] >= 4.0 * m["deviation"], f"min |pre| {m['min_abs']:.4f} < 4 x the rounding's deviation {m['deviation']:.4f}"
    assert 0.25 <= m["positive"] <= 0.75, m["positive"]
    assert m["varying_planes"] >= 0.90, m["varying_planes"]


@pytest.mark.parametrize("case_id", IDS)
def test_yardstick_is_inside_the_caps_and_not_zero(case_id):
    case, ref = H.case_by_id(case_id), H.case_reference(case_id)
    assert set(ref.yard) == set(H.names_of(case))
    for name, figs in ref.yard.items():
        print(case_id, name, {k: "%.2e" % v[0] for k, v in figs.items()})
        assert tuple(figs) == H.FIGURES[H.kind_of(name)]
        for fig, (v, _) in figs.items():
            assert v > 0.0, (name, fig)
        assert H.FACTOR["l2"] * figs["l2"][0] <= H.CAP_L2, (name, figs["l2"])


@pytest.mark.parametrize("case_id", IDS)
def test_plan_puts_the_case_on_its_path(case_id):
    case = H.case_by_id(case_id)
    plan = H.check_plan(case)
    Bt, P, steps = H.case_dims(case)
    print(case_id, plan, "steps", steps)
    assert steps == Bt * math.ceil(P / 32)
    if case.loop:
        assert plan.dh_route == "FUSED" and plan.dh_blocks == 256 and plan.s2b == 256
    if case.id == "vitb-C768":
        assert plan.dh_route == "TILES" and plan.wgrad_single == "GROUPED" and plan.s2b == plan.s1       # d W2b: a launch of its own
    if case.id == "linear-pair-grouped":
        assert steps >= 1200 and plan.s1 == 256                                                          # the 768-block split target


def test_head_plan_refuses_what_the_head_refuses():
    from depthg_amd import ops
    for B, C, D, P in ((0, 384, 70, 400), (2, 380, 70, 400), (2, 776, 70, 400), (2, 384, 129, 400), (2, 384, 70, 0)):
        with pytest.raises(RuntimeError, match="dg_head_plan_describe"):
            ops.head_plan(B, C, D, P)
    plan = ops.head_plan(64, 384, 70, 784)              # 2 x 32 images of 28 x 28: every k_head_dh2 block walks 3 or 4 tiles
    assert plan.dh_route == "FUSED" and plan.dh_blocks == 256 and plan.tiles == 13 and plan.wgrad_pair == "ONE_PASS" and plan.step_major


@pytest.mark.parametrize("case_id", ["odd-15x15", "linear-pair-grouped"])
def test_manual_backward_restates_autograd(case_id):
    """head_manual without rounding is the truth: the yardstick differs from it by the roundings alone."""
    case, ref = H.case_by_id(case_id), H.case_reference(case_id)
    man = H.head_manual(ref.inp, lambda t: t)
    for name in H.names_of(case):
        figs = H.tensor_errors(man[name].reshape(ref.truth[name].shape), ref.truth[name], H.kind_of(name))
        assert all(v < 1e-12 for v, _ in figs.values()), (name, figs)
    assert all(t.dtype == torch.float64 for t in ref.truth.values() if t is not None)
    assert ref.inp.feat.dtype == torch.float32 and set(ref.inp.keeps[1].unique().tolist()) == {0.0, 1.0}
    assert torch.equal(ref.inp.keeps[1][0], ref.inp.keeps[1][H.PATTERNS]) and not torch.equal(ref.inp.keeps[1][0], ref.inp.keeps[1][1])


def test_random_inputs_do_flip_masks():
    """What tests/test_gpu_head.py feeds does not pass mask_report: the recipe is what keeps the masks."""
    case = H.case_by_id("odd-15x15")
    g = torch.Generator().manual_seed(3)
    inp = H.case_inputs(case)._replace(feat=torch.randn(6, 384, 15, 15, generator=g) * 2.0, b2a=torch.randn(384, generator=g) * 0.05)
    ref = H.truth_f64(inp)
    m = H.mask_report(ref, H.head_manual(inp, H.to_bf16))
    assert m["flips"] > 0 and m["min_abs"] < 1e-3


def test_bf16_rounding_is_the_kernels():
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3, 0.0], dtype=torch.float64)
    assert H.to_bf16(t).tolist() == [1.0, 1.0 + 2.0 ** -6, float(torch.tensor(-0.3).bfloat16()), 0.0]      # round to nearest even


# ---- the figures measure what they say ----------------------------------------------------------------------------------------------
def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("kind,shape", [("weight", (12, 9)), ("weight", (12, 9, 1, 1)), ("bias", (11,)), ("code", (2, 5, 4, 3))])
def test_figures_are_zero_on_equal_tensors(kind, shape):
    t = _rand(shape, 0)
    for other in (t.clone(), t.float()):
        figs = H.tensor_errors(other, other.clone(), kind)
        assert tuple(figs) == H.FIGURES[kind] and all(v == 0.0 for v, _ in figs.values())


def test_figures_find_one_scaled_weight_row_and_column():
    want = _rand((10, 8), 1)
    want = want / want.norm(dim=1, keepdim=True)                                    # rows of unit norm
    got = want.clone()
    got[7] *= 1.02
    f = H.tensor_errors(got, want, "weight")
    assert f["row"][0] == pytest.approx(0.02, rel=1e-9) and f["row"][1] == (7,)
    assert f["l2"][0] == pytest.approx(0.02 / math.sqrt(10), rel=1e-9)
    assert f["elem"][1][0] == 7 and 0.0 < f["col"][0] < 0.02
    want = want / want.norm(dim=0, keepdim=True)                                    # columns of unit norm
    got = want.clone()
    got[:, 3] *= 0.99
    f = H.tensor_errors(got.reshape(10, 8, 1, 1), want.reshape(10, 8, 1, 1), "weight")
    assert f["col"][0] == pytest.approx(0.01, rel=1e-9) and f["col"][1] == (3,) and f["elem"][1][1] == 3


def test_figures_find_one_element():
    want = _rand((9,), 2)
    got = want.clone()
    got[4] += 0.5
    f = H.tensor_errors(got, want, "bias")
    assert f["elem"] == (pytest.approx(0.5 / float(want.abs().max()), rel=1e-12), (4,))
    assert f["l2"][0] == pytest.approx(0.5 / float(want.norm()), rel=1e-12)


def test_figures_find_one_code_row_and_plane():
    want = _rand((3, 7, 5, 4), 3)
    want = want / want.norm(dim=1, keepdim=True)
    got = want.clone()
    got[1, :, 2, 3] *= 1.02
    f = H.tensor_errors(got, want, "code")
    assert f["row"][0] == pytest.approx(0.02, rel=1e-9) and f["row"][1] == (1, 2, 3) and f["elem"][1][0::2] == (1, 2)
    want = want / want.norm(dim=(2, 3), keepdim=True)
    got = want.clone()
    got[2, 5] *= 0.99
    f = H.tensor_errors(got, want, "code")
    assert f["plane"][0] == pytest.approx(0.01, rel=1e-9) and f["plane"][1] == (2, 5)


def test_compare_reports_a_planted_defect():
    """The criterion end to end on the CPU: the truth itself passes, the truth with one weight row 3 % off does not."""
    case = H.case_by_id("odd-15x15")
    ref = H.case_reference(case.id)
    got = {name: ref.truth[name].clone() for name in H.names_of(case)}
    lines, bad = H.compare(case, got)
    assert not bad and len(lines) == 4 * 3 + 2 * 3 + 4
    got["cluster2.0.weight"][17] *= 1.03
    _, bad = H.compare(case, got)
    assert {(n, f) for n, f, *_ in bad} >= {("cluster2.0.weight", "row")} and all(n == "cluster2.0.weight" for n, *_ in bad)
    assert [w for n, f, _, _, w in bad if f == "row"] == [(17,)]
