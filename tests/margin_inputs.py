"""Inputs, reference and yardstick for the per-row check of the correlation loss's code gradient (tests/test_gpu_grad_margin.py,
tests/test_margin_inputs_cpu.py).  Not imported by the product.

The gradient of the loss (src/modules.py:1231-1254) is discontinuous in the code correlation cd through the clamp mask
1[lo <= cd <= hi]; on random code maps the kernels' fp16 cd flips about 5e-4 of the masks and the suite can bound the gradient by a
few percent of its L2 norm only (header of tests/test_gpu_parity.py).  Here the discontinuity is taken out from the input side:

    inputs      code maps whose normalised vectors sit close to K prototypes with pairwise |dot| in [0.12, 0.68], sampled on
                whole pixels: every cd is about +-[0.12, 0.68] or about 1, at least 0.05 away from the clamp bounds 0 and 0.8, so no
                rounding of the operands and no summation order can flip a mask (margin_report, pinned on the CPU).
    truth       oracle.depthg_oracle.forward / total_loss on float64 inputs (oracle_f64).
    yardstick   the same float64 oracle with the operands rounded the way the kernels round them - normalised feats to bf16,
                normalised code to fp16 - against the unrounded one (operand_yardstick): the error the operand formats force on any
                kernel, no GPU involved.
    figures     grad_errors: relative L2 of the whole tensor, worst position row, worst channel plane, worst element.
    criterion   every figure of the kernel's gradient <= FACTOR[family][figure] x the yardstick's, and below the caps CAP_*.
    total       the backward starts at the fused `loss.total`, which is held to the oracle's total: the weights, shifts,
                correspondence_weight and lhp balance of a recipe (WEIGHTS) are part of both the truth and the yardstick.

The constants FACTOR come from one run of the table on an MI355X (profiles/grad_margin.md holds the ratios): the worst ratio of a
route family x 1.5, rounded up to one digit.  A case added to a family later is held to the family's factor as it stands.
"""
import contextlib
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import depthg_oracle as O

FIGURES = ("l2", "row", "channel", "elem")
GradErrors = namedtuple("GradErrors", FIGURES)

# kernel figure <= FACTOR x yardstick figure, per route family (measured ratios: profiles/grad_margin.md)
FACTOR = {
    "identity": GradErrors(l2=20.0, row=20.0, channel=20.0, elem=30.0),      # worst ratios 10.3 / 10.3 / 12.5 / 14.9 (d/d code, i.i.d. feats)
    "taps": GradErrors(l2=3.0, row=3.0, channel=3.0, elem=3.0),              # 1.92 / 1.59 / 1.83 / 1.46
    "main": GradErrors(l2=3.0, row=3.0, channel=3.0, elem=4.0),              # 1.89 / 1.60 / 1.89 / 2.10
    "small": GradErrors(l2=2.0, row=2.0, channel=3.0, elem=3.0),             # 1.17 / 1.08 / 1.42 / 1.54
    "wide-identity": GradErrors(l2=5.0, row=5.0, channel=6.0, elem=6.0),     # 2.98 / 3.15 / 3.76 / 3.65 (C > 768, dense grid in channel chunks)
    "wide-taps": GradErrors(l2=4.0, row=4.0, channel=4.0, elem=4.0),         # 2.02 / 2.52 / 2.40 / 2.39 (C > 768, sampled grid in channel chunks)
}
# whatever the ratios: whole-tensor L2 at most what the exact-mask tests reach, worst row / channel at most 2e-2
CAP_L2 = {"code": 2e-3, "code_pos": 3e-3}
CAP_ROW = CAP_CHANNEL = 2e-2


# ---- the table of cases (shared by the CPU and the GPU test) --------------------------------------------------------------------
# coords: "identity" = forward_with(..., shared_coords=True, identity_grid=True) on the S == h == w grid;
#         "whole"    = coords1 != coords2 from whole_pixel_coords, not shared
#         "shared"   = ONE whole_pixel_coords grid for both coordinate sets and every image: forward_with(..., shared_coords=True)
#         "line"     = the (B, S, 1, 2) grid of depth_sampling='simple' on whole pixels, coords1 != coords2
# depth_term: cfg.depth_feat_correlation_loss (off: the 6-tuple); code_hw: side of the code maps where it is not hw (then
#         (code_hw - 1) % (hw - 1) == 0: a whole feature pixel is a whole code pixel); over: further cfg keys (weights, shifts, lhp,
#         dg_exact_masks); chunks: launch sets the call runs (channel chunks of a map wider than 768)
# seed:   fixed per case, chosen so that margin_report meets tests/test_margin_inputs_cpu.py (a condition on the inputs)
Case = namedtuple("Case", "id family kernel B C D hw S N seed pointwise zero_clamp stabalize dup coords note depth_term code_hw over chunks")


def _case(id, family, kernel, B, C, D, hw, N, seed, note, S=None, pointwise=True, zero_clamp=True, stabalize=False, dup=False,
          coords="identity", depth_term=True, code_hw=None, over=None, chunks=1):
    return Case(id, family, kernel, B, C, D, hw, hw if S is None else S, N, seed, pointwise, zero_clamp, stabalize, dup, coords, note,
                depth_term, code_hw, dict(over or {}), chunks)


# the weights case: lhp balance on, correspondence_weight != 1, four distinct weights and non-default shifts - a swapped, missing or
# forgotten factor of the fused total (DG_OUT_TOTAL) changes `loss.total` and the gradient through it by percents
WEIGHTS = dict(lhp=True, lhp_weight=0.3, lhp_weight_balance=True, correspondence_weight=1.3,
               pos_intra_weight=0.9, pos_inter_weight=0.4, neg_inter_weight=0.7, depth_feat_weight=0.23,
               pos_intra_shift=0.12, pos_inter_shift=0.05, neg_inter_shift=0.5, depth_feat_shift=0.06)


CASES = [
    # dense identity grid, k_corr2
    _case("corr2-13x13", "identity", "k_corr2", 3, 384, 70, 13, 1, 1, "P = 169, Ppad 192: the smallest map, ragged everything"),
    _case("corr2-13x13-nofold", "identity", "k_corr2", 3, 384, 70, 13, 1, 1, "the same without pointwise: no fold", pointwise=False),
    _case("corr2-20x20", "identity", "k_corr2", 9, 384, 80, 20, 2, 2, "12.5 tiles, widest code, B not a multiple of 8"),
    _case("corr2-20x20-dup", "identity", "k_corr2", 9, 384, 80, 20, 2, 2, "the same with duplicate-heavy batch maps", dup=True),
    _case("corr2-16x16", "identity", "k_corr2", 5, 384, 16, 16, 3, 3, "exactly one full row block; D of one k-step"),
    _case("corr2-32x32", "identity", "k_corr2", 2, 384, 64, 32, 2, 4, "no padded positions in the last tile"),
    _case("corr2-32x32-nofold", "identity", "k_corr2", 2, 384, 64, 32, 2, 4, "the same without pointwise: no fold", pointwise=False),
    _case("corr2-C130", "identity", "k_corr2", 2, 130, 24, 14, 1, 5, "C padded to 384"),
    _case("corr2-B1", "identity", "k_corr2", 1, 384, 70, 16, 5, 6, "one image: every negative is the image itself (quirk Q6)"),
    # k_corr2 off the identity grid: taps scatter, no fp16 gradient tiles
    _case("corr2-taps", "taps", "k_corr2", 2, 384, 70, 14, 2, 7, "coords1 != coords2 on whole pixels", S=14, coords="whole"),
    # k_corr_main above 160 positions (the exact-mask flag is refused there)
    _case("main-C768-D100", "main", "k_corr_main", 2, 768, 100, 14, 2, 8, "ViT-B widths"),
    _case("main-stabalize", "main", "k_corr_main", 3, 384, 70, 13, 1, 9, "hi = 0.8: all three mask classes", stabalize=True),
    _case("main-B66", "main", "k_corr_main", 66, 48, 33, 13, 1, 10, "a second 64-image chunk"),
    _case("main-C768-D100-noclamp", "main", "k_corr_main", 2, 768, 100, 14, 2, 8, "control: no mask at all", zero_clamp=False),
    # small grid (exact masks already): cross-check of the yardstick
    _case("small-S9", "small", "k_corr_small", 3, 64, 33, 12, 2, 11, "fused small-grid kernel", S=9, coords="whole"),
    # C > 768 on the dense identity grid: channel chunks of unit vectors (dg_normalize_split + DG_FEATS_UNIT), loss means and
    # gradients summed over the chunks
    _case("wide-id-C1536", "wide-identity", "k_corr_main", 2, 1536, 24, 14, 1, 21, "two chunks of 768", chunks=2),
    _case("wide-id-C1536-nopointwise", "wide-identity", "k_corr_main", 2, 1536, 24, 14, 1, 21, "the same without pointwise", pointwise=False, chunks=2),
    _case("wide-id-C1536-weights", "wide-identity", "k_corr_main", 2, 1536, 24, 14, 1, 21, "the same with the weights case: lhp balance on every chunk",
          over=WEIGHTS, chunks=2),
    _case("wide-id-C800", "wide-identity", "k_corr_main", 3, 800, 70, 13, 2, 22, "chunks of 400: no multiple of 128", chunks=2),
    _case("wide-id-C800-stabalize", "wide-identity", "k_corr_main", 3, 800, 70, 13, 2, 22, "the same with hi = 0.8", stabalize=True, chunks=2),
    _case("wide-id-C2048-B1", "wide-identity", "k_corr_main", 1, 2048, 70, 13, 2, 25, "three chunks (688 + 688 + 672); the image is its own negative",
          chunks=3),
    # C > 768 on sampled coordinates above 160 positions: norms over all chunks first (dg_sampled_sumsq), then dg_corr_forward_extnorm
    _case("wide-taps-C1024", "wide-taps", "k_corr_main", 2, 1024, 70, 14, 2, 23, "coordinates per image: the negatives are operands of their own",
          S=14, coords="whole", chunks=2),
    _case("wide-taps-C1024-shared", "wide-taps", "k_corr_main", 2, 1024, 70, 14, 2, 23, "one shared grid: the negatives go through the batch maps",
          S=14, coords="shared", chunks=2),
    _case("wide-taps-C1024-weights", "wide-taps", "k_corr_main", 2, 1024, 70, 14, 2, 23, "coordinates per image with the weights case",
          S=14, coords="whole", over=WEIGHTS, chunks=2),
    # C <= 768: the recipe switches and launch routes the table above does not reach
    _case("corr2-13x13-nodepth", "identity", "k_corr2", 3, 384, 70, 13, 1, 1, "no depth term: the 6-tuple", depth_term=False),
    _case("main-C768-D100-nodepth", "main", "k_corr_main", 2, 768, 100, 14, 2, 8, "no depth term", depth_term=False),
    _case("small-S9-nodepth", "small", "k_corr_small", 3, 64, 33, 12, 2, 11, "no depth term", S=9, coords="whole", depth_term=False),
    _case("ident-stabalize-C384", "main", "k_corr_main", 2, 384, 70, 13, 2, 24, "hi = 0.8 on the dense identity grid", stabalize=True),
    _case("small-code13-feats7", "small", "k_corr_small", 3, 64, 33, 7, 2, 26, "code maps 13 x 13 on feature maps 7 x 7", S=6, coords="whole", code_hw=13),
    _case("code27-feats14", "taps", "k_corr2", 2, 384, 70, 14, 2, 27, "code maps 27 x 27 on feature maps 14 x 14, 196 positions", S=14, coords="whole",
          code_hw=27),
    _case("small-line-S8", "small", "k_corr_small", 4, 48, 16, 10, 2, 28, "the S x 1 grid of depth_sampling='simple'", S=8, coords="line"),
    _case("small-shared-dup", "small", "k_corr_small", 4, 64, 33, 12, 2, 29, "one shared non-identity grid, duplicate-heavy batch maps", S=9,
          coords="shared", dup=True),
    _case("corr2-13x13-exact", "identity", "k_corr2", 3, 384, 70, 13, 1, 1, "cfg.dg_exact_masks: the same bounds as the default kernels",
          over=dict(dg_exact_masks=True)),
    _case("corr2-14x14-weights", "identity", "k_corr2", 2, 384, 70, 14, 2, 30, "the weights case on a map the kernels hold whole", over=WEIGHTS),
    _case("small-S9-weights", "small", "k_corr_small", 3, 64, 33, 12, 2, 11, "the weights case on the small grid", S=9, coords="whole", over=WEIGHTS),
]
PROTOTYPES = 4          # K of margin_code_maps in every case
FEATS_SIGMA = 0.5       # noise of the feature maps (case_inputs)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def margin_code_maps(B, D, h, w, K, seed, sigma=0.02):
    """code, code_pos (B, D, h, w) fp32 from float64 arithmetic: every position is one of K unit prototypes (a 3-dimensional
    subspace, pairwise |dot| in [0.12, 0.68], embedded in the D channels through a random orthonormal D x 3 matrix so that every
    channel is populated) plus sigma x a random unit vector, times a random scale in [0.5, 2] (so that the Jacobian of the
    normalisation matters).  Both maps use the same prototypes and embedding."""
    g = torch.Generator().manual_seed(seed)
    while True:
        proto = _unit(torch.randn(K, 3, generator=g, dtype=torch.float64))
        off = (proto @ proto.t()).abs()[~torch.eye(K, dtype=torch.bool)]
        if float(off.min()) >= 0.12 and float(off.max()) <= 0.68:
            break
    q, _ = torch.linalg.qr(torch.randn(D, 3, generator=g, dtype=torch.float64))          # D x 3, orthonormal columns
    emb = proto @ q.t()                                                                   # K x D unit vectors
    maps = []
    for _ in range(2):
        pick = torch.randint(0, K, (B, h, w), generator=g)
        noise = _unit(torch.randn(B, h, w, D, generator=g, dtype=torch.float64))
        scale = 0.5 + 1.5 * torch.rand(B, h, w, 1, generator=g, dtype=torch.float64)
        maps.append(((emb[pick] + sigma * noise) * scale).permute(0, 3, 1, 2).contiguous().to(torch.float32))
    return maps[0], maps[1]


def _pixel_coordinate(idx, size):
    """The float32 c whose unnormalisation ((c + 1) / 2) * (size - 1) in float32 (grid_sample(align_corners=True) as
    O.bilinear_taps writes it) lies closest to idx: the float32 nearest -1 + 2 idx / (size - 1) or one of its two neighbours.
    Not every pixel has a float32 coordinate that unnormalises to it exactly; the rest is below 1e-6 of a pixel."""
    c = np.float32(-1.0 + 2.0 * idx / (size - 1))
    cands = (c, np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-2)))
    err = [abs(float(((k + np.float32(1.0)) / np.float32(2.0)) * np.float32(size - 1)) - idx) for k in cands]
    assert min(err) < 1e-6 * max(idx, 1)
    return cands[int(np.argmin(err))]


def whole_pixel_coords(B, S, h, w, seed, Sh=None):
    """coords (B, S, S, 2) in [-1, 1] that land on pixel centres - a random selection of the h x w pixels per image, repeats
    allowed - so that the bilinear `sample` never mixes two prototypes (a neighbouring pixel enters with a weight below 1e-6,
    where float32 has no coordinate for the centre itself).  Sh: the grid's second extent where it is not S (1: the line grid)."""
    g = torch.Generator().manual_seed(seed)
    xs = np.asarray([_pixel_coordinate(i, w) for i in range(w)], dtype=np.float32)
    ys = np.asarray([_pixel_coordinate(i, h) for i in range(h)], dtype=np.float32)
    ix = torch.randint(0, w, (B, S, S if Sh is None else Sh), generator=g)
    iy = torch.randint(0, h, (B, S, S if Sh is None else Sh), generator=g)
    return torch.stack([torch.from_numpy(xs)[ix], torch.from_numpy(ys)[iy]], dim=-1)


def iid_feats(case):
    """Which feature maps a case gets.  Structured ones (margin_code_maps with half a unit of noise) by default: like a backbone's
    features they give correlations fd with structure, not 1 / sqrt(C) noise, and the rounding of the operands stays small against
    the gradient (with i.i.d. features d/d code_pos, which only the inter pair-set with its shift of 0.02 feeds, is a sum of
    cancelling terms, and its yardstick reaches 1.3e-2 - 1.6e-2 on the worst row at C <= 64).  The identity grids without padded
    positions are held to the 2e-5 bound of test_dense_grids_without_padded_positions on the loss means, which presumes what that
    test feeds: i.i.d. features, whose rounding errors average out over the B P P elements of a mean (structured features make them
    coherent: the float64 yardstick alone is 2e-5 .. 5e-4 off on these means) - they get i.i.d. features."""
    return case.coords == "identity" and case.hw % 8 == 0


def case_cfg(case, **over):
    return O.default_cfg(**{**dict(feature_samples=case.S, neg_samples=case.N, dim=case.D, dg_outputs="reduced", pointwise=case.pointwise,
                                   zero_clamp=case.zero_clamp, stabalize=case.stabalize, depth_feat_correlation_loss=case.depth_term),
                            **case.over, **over})


def case_inputs(case):
    """(feats, feats_pos, code, code_pos, depth, coords1, coords2, perms) of a case, fp32 on the CPU."""
    B, C, D, hw, S, N = case.B, case.C, case.D, case.hw, case.S, case.N
    g = torch.Generator().manual_seed(7000 + case.seed)
    if iid_feats(case):
        f, fp = torch.randn(B, C, hw, hw, generator=g), torch.randn(B, C, hw, hw, generator=g)
    else:
        f, fp = margin_code_maps(B, C, hw, hw, PROTOTYPES, 900 + case.seed, sigma=FEATS_SIGMA)
    d = torch.randint(0, 256, (B, 1, 4 * hw, 4 * hw), generator=g).float()
    d[:, :, :7, :9] = 0.0
    if case.dup:          # many negatives on the same few images (super_perm's output need not be a permutation, quirk Q6)
        perms = [torch.randint(0, 3, (B,), generator=g) for _ in range(N)]
    else:
        perms = [O.super_perm(B, g) for _ in range(N)]
    hc = hw if case.code_hw is None else case.code_hw
    assert (hc - 1) % (hw - 1) == 0, "a whole feature pixel must be a whole code pixel"
    c, cp = margin_code_maps(B, D, hc, hc, PROTOTYPES, case.seed)
    if case.coords == "identity":
        c1 = c2 = O.identity_coords(B, S)
    elif case.coords == "shared":
        c1 = c2 = whole_pixel_coords(1, S, hw, hw, 100 + case.seed).expand(B, S, S, 2).contiguous()
    else:
        Sh = 1 if case.coords == "line" else None
        c1, c2 = whole_pixel_coords(B, S, hw, hw, 100 + case.seed, Sh), whole_pixel_coords(B, S, hw, hw, 200 + case.seed, Sh)
    return f, fp, c, cp, d, c1, c2, perms


# ---- reference and yardstick ----------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _norm_hook(fn):
    """O.norm replaced by fn(O.norm(t), t) for the duration of the block (helper / depth_feature_correlation look the name up at
    call time); oracle/ itself is not changed."""
    orig = O.norm
    O.norm = lambda t: fn(orig(t), t)
    try:
        yield
    finally:
        O.norm = orig


def _round_like_the_kernels(n, src):
    """The operand formats of the kernels (header of tests/test_gpu_parity.py): normalised code to fp16, normalised feats (and the
    depth indicators, which are 0 / +-1 and survive) to bf16.  Code is what carries a gradient here; its rounding is invisible to
    the backward (the kernels apply the Jacobian of the normalisation to the gradient the rounded operands give)."""
    if src.requires_grad:
        return n + (n.detach().to(torch.float16).to(n.dtype) - n.detach())
    return n.to(torch.bfloat16).to(n.dtype)


def _round_code_only(n, src):
    return _round_like_the_kernels(n, src) if src.requires_grad else n


def oracle_f64(cfg, f, fp, c, cp, d, c1, c2, perms, hook=None):
    """oracle.depthg_oracle.forward / total_loss on .double() inputs -> (tuple, total, d/d code, d/d code_pos), all float64.
    hook: a function for _norm_hook (the yardstick's rounding)."""
    cr, cpr = c.double().requires_grad_(True), cp.double().requires_grad_(True)
    with _norm_hook(hook) if hook is not None else contextlib.nullcontext():
        out = O.forward(cfg, f.double(), fp.double(), cr, cpr, d.double(), d.double(), coords1=c1, coords2=c2, perms=perms)
        total = O.total_loss(cfg, out)
        total.backward()
    return tuple(o.detach() for o in out), total.detach(), cr.grad, cpr.grad


def _classes(cfg, cd):
    """Mask class of every element: 0 below lo, 1 inside [lo, hi], 2 above hi (only the finite bounds count)."""
    cls = torch.ones_like(cd, dtype=torch.int8)
    if cfg.zero_clamp:
        cls[cd < 0.0] = 0
    if cfg.stabalize:
        cls[cd > 0.8] = 2
    return cls


def margin_report(cfg, f, fp, c, cp, d, c1, c2, perms, ref=None):
    """From the float64 reference alone, over every pair-set (intra, inter, each negative):
        margin   the smallest distance of a cd to a finite clamp bound (0 with zero_clamp, 0.8 with stabalize; inf without either)
        shares   {pair-set: share of its elements per mask class that the recipe can produce (below lo, inside, above hi)}
        flips    the number of masks that change when the normalised code is rounded to fp16"""
    ref = ref if ref is not None else oracle_f64(cfg, f, fp, c, cp, d, c1, c2, perms)
    rnd = oracle_f64(cfg, f, fp, c, cp, d, c1, c2, perms, hook=_round_code_only)
    B = c.shape[0]
    sets = {"intra": (ref[0][1], rnd[0][1]), "inter": (ref[0][3], rnd[0][3])}
    for k in range(int(cfg.neg_samples)):
        sets[f"neg{k}"] = (ref[0][5][k * B:(k + 1) * B], rnd[0][5][k * B:(k + 1) * B])
    bounds = ([0.0] if cfg.zero_clamp else []) + ([0.8] if cfg.stabalize else [])
    wanted = ([0] if cfg.zero_clamp else []) + [1] + ([2] if cfg.stabalize else [])
    margin, flips, shares = float("inf"), 0, {}
    for name, (cd, cd_r) in sets.items():
        for bnd in bounds:
            margin = min(margin, float((cd - bnd).abs().min()))
        cls = _classes(cfg, cd)
        flips += int((cls != _classes(cfg, cd_r)).sum())
        shares[name] = [float((cls == k).double().mean()) for k in wanted]
    return {"margin": margin, "flips": flips, "shares": shares}


def grad_errors(got, want):
    """The four figures of a gradient (B, D, h, w) against its reference:
        l2       ||got - want|| / ||want||
        row      max over (b, y, x) of ||got - want||_2 over the channels / RMS of the reference's row norms
        channel  max over (b, d) of ||got - want||_2 over the plane / RMS of the reference's plane norms
        elem     max |got - want| / max |want|"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    diff = got - want
    rms = lambda t: float(t.square().mean().sqrt())
    return GradErrors(l2=float(diff.norm() / want.norm()),
                      row=float(diff.norm(dim=1).max()) / rms(want.norm(dim=1)),
                      channel=float(diff.norm(dim=(2, 3)).max()) / rms(want.norm(dim=(2, 3))),
                      elem=float(diff.abs().max() / want.abs().max()))


def worst_locations(got, want):
    """Where grad_errors found its worst row (b, y, x), channel plane (b, d) and element (b, d, y, x): they locate a defect to a
    tile and a pair-set."""
    diff = got.detach().double().cpu() - want.detach().double().cpu()
    at = lambda t: tuple(int(v) for v in np.unravel_index(int(t.argmax()), t.shape))
    return {"row": at(diff.norm(dim=1)), "channel": at(diff.norm(dim=(2, 3))), "elem": at(diff.abs())}


def operand_yardstick(cfg, f, fp, c, cp, d, c1, c2, perms, ref=None):
    """grad_errors of the float64 oracle run on operands rounded as the kernels round them, against the unrounded run:
    {"code": GradErrors, "code_pos": GradErrors}."""
    ref = ref if ref is not None else oracle_f64(cfg, f, fp, c, cp, d, c1, c2, perms)
    rnd = oracle_f64(cfg, f, fp, c, cp, d, c1, c2, perms, hook=_round_like_the_kernels)
    return {"code": grad_errors(rnd[2], ref[2]), "code_pos": grad_errors(rnd[3], ref[3])}


@functools.lru_cache(maxsize=None)
def case_reference(case_id):
    """(cfg, inputs, oracle_f64 result) of a case, computed once per process and shared; nobody writes into it."""
    case = next(k for k in CASES if k.id == case_id)
    cfg, inp = case_cfg(case), case_inputs(case)
    return cfg, inp, oracle_f64(cfg, *inp)
