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

The constants FACTOR come from one run of the table on an MI355X (profiles/grad_margin.md holds the ratios): the worst ratio of a
route family x 1.5, rounded up to one digit.
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
}
# whatever the ratios: whole-tensor L2 at most what the exact-mask tests reach, worst row / channel at most 2e-2
CAP_L2 = {"code": 2e-3, "code_pos": 3e-3}
CAP_ROW = CAP_CHANNEL = 2e-2


# ---- the table of cases (shared by the CPU and the GPU test) --------------------------------------------------------------------
# coords: "identity" = forward_with(..., shared_coords=True, identity_grid=True) on the S == h == w grid;
#         "whole"    = coords1 != coords2 from whole_pixel_coords, not shared
# seed:   fixed per case, chosen so that margin_report meets tests/test_margin_inputs_cpu.py (a condition on the inputs)
Case = namedtuple("Case", "id family kernel B C D hw S N seed pointwise zero_clamp stabalize dup coords note")


def _case(id, family, kernel, B, C, D, hw, N, seed, note, S=None, pointwise=True, zero_clamp=True, stabalize=False, dup=False,
          coords="identity"):
    return Case(id, family, kernel, B, C, D, hw, hw if S is None else S, N, seed, pointwise, zero_clamp, stabalize, dup, coords, note)


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


def whole_pixel_coords(B, S, h, w, seed):
    """coords (B, S, S, 2) in [-1, 1] that land on pixel centres - a random selection of the h x w pixels per image, repeats
    allowed - so that the bilinear `sample` never mixes two prototypes (a neighbouring pixel enters with a weight below 1e-6,
    where float32 has no coordinate for the centre itself)."""
    g = torch.Generator().manual_seed(seed)
    xs = np.asarray([_pixel_coordinate(i, w) for i in range(w)], dtype=np.float32)
    ys = np.asarray([_pixel_coordinate(i, h) for i in range(h)], dtype=np.float32)
    ix = torch.randint(0, w, (B, S, S), generator=g)
    iy = torch.randint(0, h, (B, S, S), generator=g)
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
    return O.default_cfg(feature_samples=case.S, neg_samples=case.N, dim=case.D, dg_outputs="reduced", pointwise=case.pointwise,
                         zero_clamp=case.zero_clamp, stabalize=case.stabalize, **over)


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
    c, cp = margin_code_maps(B, D, hw, hw, PROTOTYPES, case.seed)
    if case.coords == "identity":
        c1 = c2 = O.identity_coords(B, S)
    else:
        c1, c2 = whole_pixel_coords(B, S, hw, hw, 100 + case.seed), whole_pixel_coords(B, S, hw, hw, 200 + case.seed)
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
