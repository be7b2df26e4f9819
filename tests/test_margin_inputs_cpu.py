"""CPU side of the per-row gradient check (tests/margin_inputs.py): the inputs of every case of tests/test_gpu_grad_margin.py keep
every code correlation away from the clamp bounds, the error figures measure what they say, and the operand yardstick is a small,
non-zero number.  No GPU, float64 oracle only."""
import pytest
import torch

import margin_inputs as M

IDS = [c.id for c in M.CASES]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(16)


@pytest.mark.parametrize("case_id", IDS)
def test_case_inputs_cannot_flip_a_mask(case_id):
    """A condition on the inputs (the seeds of the table are chosen for it): no cd of any pair-set within 0.05 of a finite clamp
    bound, no mask changed by rounding the normalised code to fp16, every mask class the recipe can produce >= 10 % of every
    pair-set."""
    cfg, inp, ref = M.case_reference(case_id)
    rep = M.margin_report(cfg, *inp, ref=ref)
    print(case_id, "margin %.3f" % rep["margin"], "flips", rep["flips"], {k: ["%.3f" % s for s in v] for k, v in rep["shares"].items()})
    assert rep["margin"] >= 0.05
    assert rep["flips"] == 0
    assert set(rep["shares"]) == {"intra", "inter"} | {f"neg{k}" for k in range(int(cfg.neg_samples))}
    for name, shares in rep["shares"].items():
        assert len(shares) == int(cfg.zero_clamp) + 1 + int(cfg.stabalize)
        assert min(shares) >= 0.10, (name, shares)
        assert sum(shares) == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize("case_id", IDS)
def test_operand_yardstick_is_small_and_not_zero(case_id):
    cfg, inp, ref = M.case_reference(case_id)
    yard = M.operand_yardstick(cfg, *inp, ref=ref)
    print(case_id, {k: ["%.2e" % v for v in g] for k, g in yard.items()})
    for name in ("code", "code_pos"):
        for fig, v in zip(M.FIGURES, yard[name]):
            assert 0.0 < v < 1e-2, (name, fig, v)


def test_table_reaches_every_route_and_recipe_switch():
    """The table itself: unique ids, and at least one case per launch route and recipe switch of the correlation loss."""
    assert len(set(IDS)) == len(IDS)
    has = lambda pred: any(pred(c) for c in M.CASES)
    wide = lambda c: c.chunks > 1
    assert has(lambda c: wide(c) and c.coords == "identity" and c.chunks == 3) and has(lambda c: wide(c) and c.coords == "whole")
    assert has(lambda c: wide(c) and c.coords == "shared") and has(lambda c: wide(c) and not c.pointwise)
    assert has(lambda c: wide(c) and c.stabalize) and has(lambda c: wide(c) and c.B == 1)
    for coords in ("identity", "whole"):          # the weights case on both wide routes, on a narrow identity grid and on the small grid
        assert has(lambda c: wide(c) and c.coords == coords and c.over.get("lhp_weight_balance"))
    assert has(lambda c: c.kernel == "k_corr2" and not wide(c) and c.over.get("lhp_weight_balance"))
    assert has(lambda c: c.kernel == "k_corr_small" and c.over.get("lhp_weight_balance"))
    for kernel in ("k_corr2", "k_corr_main", "k_corr_small"):
        assert has(lambda c: c.kernel == kernel and not c.depth_term)
    assert has(lambda c: c.code_hw is not None and c.S ** 2 <= 160) and has(lambda c: c.code_hw is not None and c.S ** 2 > 160)
    assert has(lambda c: c.coords == "line") and has(lambda c: c.coords == "shared" and c.S ** 2 <= 160 and c.dup)
    assert has(lambda c: c.over.get("dg_exact_masks") and c.coords == "identity")
    for c in M.CASES:
        assert c.family in M.FACTOR, c.id
        assert c.code_hw is None or (c.code_hw - 1) % (c.hw - 1) == 0, c.id
        assert (c.chunks > 1) == (c.C > 768 and (c.coords == "identity" or c.S ** 2 > 160)), c.id


def _weights_case():
    return next(c for c in M.CASES if c.id == "wide-id-C1536-weights")


def test_weights_case_scales_the_oracles_total_by_the_balance():
    """The semantics the GPU weights cases are held to (src/train_segmentation.py:326-335): with the depth term, lhp and
    lhp_weight_balance, EVERY term of the total is scaled by correspondence_weight - lhp_weight, so the total and both gradients are
    (correspondence_weight - lhp_weight) / correspondence_weight times those of the same inputs without balance."""
    case = _weights_case()
    cfg, inp, ref = M.case_reference(case.id)
    assert cfg.lhp and cfg.lhp_weight_balance and cfg.depth_feat_correlation_loss and cfg.correspondence_weight != 1.0
    assert len({cfg.pos_intra_weight, cfg.pos_inter_weight, cfg.neg_inter_weight, cfg.depth_feat_weight}) == 4
    plain = M.oracle_f64(M.case_cfg(case, lhp_weight_balance=False), *inp)
    factor = (cfg.correspondence_weight - cfg.lhp_weight) / cfg.correspondence_weight
    assert factor == pytest.approx(1.0 / 1.3, rel=1e-12)
    assert float(ref[1]) == pytest.approx(factor * float(plain[1]), rel=1e-12)
    for k in (2, 3):
        assert float((ref[k] - factor * plain[k]).norm()) <= 1e-12 * float(plain[k].norm())
    # the total by hand from the tuple: four distinct weights, one scale
    o = ref[0]
    by_hand = (cfg.pos_intra_weight * o[0] + cfg.pos_inter_weight * o[2] + cfg.neg_inter_weight * o[4].mean() +
               cfg.depth_feat_weight * o[6]) * (cfg.correspondence_weight - cfg.lhp_weight)
    assert float(ref[1]) == pytest.approx(float(by_hand), rel=1e-12)


def test_no_balance_without_the_depth_term():
    """With the depth term off the caller applies correspondence_weight alone (src/train_segmentation.py:337-349): the lhp keys change
    nothing, and the tuple has six elements."""
    case = _weights_case()
    _, inp, _ = M.case_reference(case.id)
    cfg_on = M.case_cfg(case, depth_feat_correlation_loss=False)
    cfg_off = M.case_cfg(case, depth_feat_correlation_loss=False, lhp=False, lhp_weight_balance=False)
    on, off = M.oracle_f64(cfg_on, *inp), M.oracle_f64(cfg_off, *inp)
    assert len(on[0]) == len(off[0]) == 6
    assert float(on[1]) == float(off[1]) and torch.equal(on[2], off[2]) and torch.equal(on[3], off[3])
    o = on[0]
    by_hand = (cfg_on.pos_intra_weight * o[0] + cfg_on.pos_inter_weight * o[2] + cfg_on.neg_inter_weight * o[4].mean()) * \
        cfg_on.correspondence_weight
    assert float(on[1]) == pytest.approx(float(by_hand), rel=1e-12)


def test_margin_report_sees_a_cd_at_the_bound():
    """Random code maps (what the other parity tests use) do not pass: cds at the bound, masks that flip in fp16."""
    case = M.CASES[0]
    cfg, inp = M.case_cfg(case), list(M.case_inputs(case))
    g = torch.Generator().manual_seed(5)
    inp[2], inp[3] = torch.randn(inp[2].shape, generator=g), torch.randn(inp[3].shape, generator=g)
    rep = M.margin_report(cfg, *inp)
    assert rep["margin"] < 1e-4 and rep["flips"] > 0


def test_margin_code_maps_construction():
    B, D, h, w, K = 3, 24, 9, 7, 4
    c, cp = M.margin_code_maps(B, D, h, w, K, seed=3)
    assert c.shape == cp.shape == (B, D, h, w) and c.dtype == torch.float32 and not torch.equal(c, cp)
    n = torch.cat([c, cp]).double().permute(0, 2, 3, 1).reshape(-1, D)
    norms = n.norm(dim=1)
    assert float(norms.min()) > 0.48 and float(norms.max()) < 2.05 and float(norms.std()) > 0.3        # the scales
    assert bool((c.abs().amax(dim=(0, 2, 3)) > 0).all())                                                # every channel populated
    cos = (n / norms[:, None]) @ (n / norms[:, None]).t()
    near_one = cos > 0.99
    cross = cos[~near_one].abs()
    assert float(cross.min()) >= 0.12 - 0.06 and float(cross.max()) <= 0.68 + 0.06
    # K groups of positions: the rank of the "same prototype" relation
    assert int(torch.linalg.matrix_rank(near_one.double())) == K
    again, _ = M.margin_code_maps(B, D, h, w, K, seed=3)
    assert torch.equal(c, again)


def test_whole_pixel_coords_land_on_pixels():
    from oracle import depthg_oracle as O
    B, S, h, w = 2, 9, 12, 14
    c = M.whole_pixel_coords(B, S, h, w, seed=1)
    assert c.shape == (B, S, S, 2) and c.dtype == torch.float32 and float(c.min()) >= -1.0 and float(c.max()) <= 1.0
    x0, y0, _, _, wx1, wy1 = O.bilinear_taps(c, h, w)
    off = torch.minimum(torch.stack([wx1, wy1]), 1.0 - torch.stack([wx1, wy1]))
    assert float(off.max()) < 1e-5                                      # at most 1e-6 of a pixel x 13
    assert len(torch.unique(x0)) > w // 2 and len(torch.unique(y0)) > h // 2
    t = torch.arange(B * h * w, dtype=torch.float64).reshape(B, 1, h, w)
    got = O.sample(t, c)
    assert float((got - got.round()).abs().max()) < 1e-2 and not torch.equal(c, M.whole_pixel_coords(B, S, h, w, seed=2))


def _unit_rows(shape, seed):
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return t / t.norm(dim=1, keepdim=True)


def test_grad_errors_zero_on_equal_tensors():
    t = _unit_rows((2, 5, 4, 3), 0)
    assert M.grad_errors(t, t.clone()) == M.GradErrors(0.0, 0.0, 0.0, 0.0)
    assert M.grad_errors(t.float(), t.float()) == M.GradErrors(0.0, 0.0, 0.0, 0.0)


def test_grad_errors_report_one_scaled_row():
    """Every row of unit norm: one row scaled by 1.02 is a worst-row figure of 0.02, a whole-tensor figure of 0.02 / sqrt(rows)."""
    want = _unit_rows((3, 7, 5, 4), 1)
    got = want.clone()
    got[1, :, 2, 3] *= 1.02
    e = M.grad_errors(got, want)
    assert e.row == pytest.approx(0.02, rel=1e-9)
    assert e.l2 == pytest.approx(0.02 / (3 * 5 * 4) ** 0.5, rel=1e-9)
    assert e.elem == pytest.approx(0.02 * float(want[1, :, 2, 3].abs().max() / want.abs().max()), rel=1e-9)
    assert 0.0 < e.channel < 0.02
    assert M.worst_locations(got, want)["row"] == (1, 2, 3)


def test_grad_errors_report_one_scaled_channel():
    """Every channel plane of unit norm: one plane scaled by 0.99 is a worst-channel figure of 0.01."""
    want = torch.randn(2, 6, 5, 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want = want / want.norm(dim=(2, 3), keepdim=True)
    got = want.clone()
    got[0, 4] *= 0.99
    e = M.grad_errors(got, want)
    assert e.channel == pytest.approx(0.01, rel=1e-9)
    assert e.l2 == pytest.approx(0.01 / (2 * 6) ** 0.5, rel=1e-9)
    loc = M.worst_locations(got, want)
    assert loc["channel"] == (0, 4) and loc["elem"][:2] == (0, 4)


def test_oracle_f64_leaves_the_oracle_as_it_was():
    from oracle import depthg_oracle as O
    before = O.norm
    case = M.CASES[0]
    cfg, inp, ref = M.case_reference(case.id)
    M.operand_yardstick(cfg, *inp, ref=ref)
    assert O.norm is before
    assert all(t.dtype == torch.float64 for t in ref[0]) and ref[2].dtype == ref[3].dtype == torch.float64
    # float64 and the suite's float32 oracle agree to float32 rounding
    f, fp, c, cp, d, c1, c2, perms = inp
    cr = c.clone().requires_grad_(True)
    out = O.forward(cfg, f, fp, cr, cp, d, d, coords1=c1, coords2=c2, perms=perms)
    O.total_loss(cfg, out).backward()
    assert M.grad_errors(cr.grad, ref[2]).l2 < 1e-5
