"""Inputs, reference and yardstick for the per-row check of the projection head's backward where its persistent kernels loop
(tests/test_gpu_head_margin.py, tests/test_head_margin_inputs_cpu.py).  Not imported by the product.

The head's gradients are discontinuous in cluster2's pre-activation through the ReLU mask; on random inputs the bf16 pre-activation
flips about 0.2 % of the masks and tests/test_gpu_head.py can hold d W2a to 6e-2 of its L2 norm only.  Here the discontinuity is
taken out from the input side, as tests/margin_inputs.py does for the clamp mask of the correlation loss:

    inputs      case_inputs: every position's feature vector is one of PROTOTYPES vectors plus NOISE x noise, cluster2's Dropout2d
                rows are PATTERNS distinct patterns dealt b % PATTERNS, so the pre-activation of a hidden channel takes
                PATTERNS x PROTOTYPES cluster values; b2a puts zero into the middle of the widest central gap between them (>= MIN_GAP)
                and between the prototypes of every pattern: both mask classes occur in every (image, channel) plane, and no rounding
                of the operands reaches zero (mask_report, pinned on the CPU).
    truth       oracle.head_oracle.head_forward on float64 tensors under autograd, summed over both passes of a pair (truth_f64).
    yardstick   head_manual: the same three products and the mask each way in float64, with every operand rounded to bf16 where the
                kernels of depthg_amd/csrc/dg_head.hip round it (the lines are cited there), against the unrounded truth: the error
                the operand formats force on any kernel, no GPU involved.  The mask is the truth's.
    figures     tensor_errors: relative L2, worst row, worst column (weights) / worst plane (code), worst element, each with where.
    criterion   every figure of the kernels <= FACTOR[figure] x the yardstick's, every L2 figure <= CAP_L2.

FACTOR is fixed in advance: the kernels add only the fp32 accumulation order to the operand roundings (2 on L2 / row / column /
plane), the worst element is an extreme value of 1e5 - 1e7 elements (3).
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import head_oracle as HO

P_DROP = 0.1
SCALE = 1.0 / (1.0 - P_DROP)
PROTOTYPES, PATTERNS, NOISE, MIN_GAP = 3, 3, 0.01, 0.4
FACTOR = {"l2": 2.0, "row": 2.0, "col": 2.0, "plane": 2.0, "elem": 3.0}
CAP_L2 = 2e-2
PARAMS = ("cluster1.0.weight", "cluster1.0.bias", "cluster2.0.weight", "cluster2.0.bias", "cluster2.2.weight", "cluster2.2.bias")
FIGURES = {"weight": ("l2", "row", "col", "elem"), "bias": ("l2", "elem"), "code": ("l2", "row", "plane", "elem")}


def kind_of(name):
    return "code" if name == "code" else ("weight" if name.endswith("weight") else "bias")


# ---- the table of cases (shared by the CPU and the GPU test) --------------------------------------------------------------------
# B: images per pass (pair: forward_pair on B + B).  dh / pair / single / step_major: what ops.head_plan must say (None: not looked
# at - the linear head has no d hidden, the nonlinear cases' lone products are not what they are about).  loop: k_head_dh2 blocks
# with three tiles.  grouped: the split count whose k_head_wgrad2 launch must cover >= 4 steps per split.
Case = namedtuple("Case", "id pair B C D hw proj seed dh wgrad_pair wgrad_single step_major loop grouped note")
CASES = [
    Case("loop-pair-20x20", True, 37, 384, 70, 20, "nonlinear", 1, "FUSED", "ONE_PASS", None, True, True, None,
         "518 tiles on 256 blocks of k_head_dh2<5>; k_head_wgrad3 step-major, 962 steps in 80 splits across image boundaries"),
    Case("loop-12x12-D96-C352", False, 180, 352, 96, 12, "nonlinear", 2, "FUSED", "ONE_PASS", None, True, True, None,
         "540 tiles on 256 blocks of k_head_dh2<6>, clamped rows of d hidden and of the last channel tile; 900 steps in 80 splits"),
    Case("fused-grouped-C256", False, 40, 256, 70, 20, "nonlinear", 3, "FUSED", "GROUPED", None, False, False, "s2a",
         "k_head_dh2 in front of k_head_wgrad2 with the second product, row-major d hidden; 520 steps in 88 splits"),
    Case("onepass-rowmajor-D100", False, 26, 384, 100, 20, "nonlinear", 4, "TILES", "ONE_PASS", None, False, False, None,
         "k_head_dh<6, 0> staged; k_head_wgrad3 on a row-major d hidden, seven d code pieces; 338 steps in 80 splits"),
    Case("linear-pair-grouped", True, 47, 384, 70, 20, "linear", 5, None, None, "GROUPED", None, False, "s1",
         "1222 steps: the split target of 768 blocks; k_head_wgrad2 fp32 x fp32 alone"),
    Case("vitb-C768", False, 8, 768, 100, 16, "nonlinear", 6, "TILES", "GROUPED", None, False, False, "s2a",
         "k_head_dh<12, 0> unstaged; the grouped pair launch with four steps per split; d W2b a launch of its own"),
    Case("odd-15x15", False, 6, 384, 70, 15, "nonlinear", 7, "TILES", "DIRECT", "DIRECT", False, False, None,
         "P = 225 off every 8-aligned path: unstaged d hidden, k_head_wgrad with guarded tails"),
]


def case_by_id(case_id):
    return next(k for k in CASES if k.id == case_id)


def case_dims(case):
    """(images in all, positions, 32-position steps in all)"""
    Bt, P = (2 if case.pair else 1) * case.B, case.hw * case.hw
    return Bt, P, Bt * ((P + 31) // 32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
Inputs = namedtuple("Inputs", "feat keeps w1 b1 w2a b2a w2b b2b up")      # feat, up: (Bt, C | D, hw, hw); keeps: three (Bt, C); fp32


def _margin_w2a(proto, patterns, C, g):
    """W2a (C, C) and b2a (C): per hidden channel m the pre-activation without noise takes the values
    v[m, r, k] = SCALE sum_c patterns[r, c] W2a[m, c] proto[k, c].  b2a[m] = minus the middle of the widest of the central gaps of the
    sorted values (at least three of the nine on either side).  A row is drawn again while that gap is below MIN_GAP or some pattern
    has all its prototypes on one side (the mask would be constant over that pattern's planes)."""
    R, K = patterns.shape[0], proto.shape[0]
    draw = lambda n: (torch.randn(n, C, generator=g, dtype=torch.float64) / math.sqrt(C)).float().double()
    W = draw(C)
    for _ in range(200):
        v = SCALE * torch.einsum("rc,mc,kc->mrk", patterns, W, proto)
        s = v.reshape(C, R * K).sort(dim=1).values
        gaps = (s[:, 1:] - s[:, :-1])[:, 2:R * K - 3]
        gap, at = gaps.max(dim=1)
        thr = 0.5 * (s.gather(1, (at + 2)[:, None]) + s.gather(1, (at + 3)[:, None]))      # (C, 1)
        above = v > thr[:, :, None]
        straddle = (above.any(dim=2) & (~above).any(dim=2)).all(dim=1)
        bad = (gap < MIN_GAP) | ~straddle
        if not bool(bad.any()):
            return W.float(), (-thr[:, 0]).float()
        W[bad] = draw(int(bad.sum()))
    raise AssertionError("no W2a with the margin found")


def case_inputs(case):
    """The inputs of a case, fp32 on the CPU, both passes of a pair stacked along the batch (the first pass's B images first)."""
    Bt, P, _ = case_dims(case)
    C, D, hw = case.C, case.D, case.hw
    g = torch.Generator().manual_seed(4000 + case.seed)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    proto = rn(PROTOTYPES, C) * 2.0
    pick = torch.randint(0, PROTOTYPES, (Bt, P), generator=g)
    feat = (proto[pick] + NOISE * rn(Bt, P, C)).permute(0, 2, 1).reshape(Bt, C, hw, hw).contiguous().float()
    while True:
        patterns = (torch.rand(PATTERNS, C, generator=g) < 1.0 - P_DROP).double()
        if len({tuple(r.tolist()) for r in patterns}) == PATTERNS:
            break
    keep2 = patterns[torch.arange(Bt) % PATTERNS].float()
    keep1, keep3 = ((torch.rand(Bt, C, generator=g) < 1.0 - P_DROP).float() for _ in range(2))
    w2a, b2a = _margin_w2a(proto, patterns, C, g)
    w1, w2b = (rn(D, C) / math.sqrt(C)).float(), (rn(D, C) / math.sqrt(C)).float()
    b1, b2b = (0.1 * rn(D)).float(), (0.1 * rn(D)).float()
    up = rn(Bt, D, hw, hw).float()
    if case.proj != "nonlinear":
        w2a = b2a = w2b = b2b = None
    return Inputs(feat, (keep1, keep2, keep3), w1, b1, w2a, b2a, w2b, b2b, up)


# ---- truth ----------------------------------------------------------------------------------------------------------------------
def truth_f64(inp):
    """oracle.head_oracle.head_forward on .double() tensors under autograd, upstream `up` on code ->
    {"code", the six (or two) parameter names: float64 gradients, "pre": cluster2's pre-activation (None for the linear head)}."""
    nl = inp.w2a is not None
    prm = [t.double().requires_grad_(True) for t in (inp.w1, inp.b1) + ((inp.w2a, inp.b2a, inp.w2b, inp.b2b) if nl else ())]
    f, keeps = inp.feat.double(), tuple(k.double() for k in inp.keeps)
    code, _ = HO.head_forward(f, *prm, keeps=keeps, p=P_DROP)
    (code * inp.up.double()).sum().backward()
    out = {"code": code.detach(), "pre": None}
    out.update({name: p.grad for name, p in zip(PARAMS, prm)})
    if nl:
        with torch.no_grad():
            out["pre"] = HO.conv1x1(f * (keeps[1] * SCALE)[:, :, None, None], prm[2], prm[3])
    return out


# ---- yardstick ------------------------------------------------------------------------------------------------------------------
def to_bf16(t):
    return t.float().bfloat16().double()


def head_manual(inp, rnd, mask=None):
    """Forward and backward of the head written out - three products and a mask each way - in float64, `rnd` applied to every operand
    where the kernels round it (rnd = identity restates the truth; tests/test_head_margin_inputs_cpu.py holds it against autograd).
    mask: the ReLU mask to use (Bt, C, hw, hw) or None for the one of this run's own pre-activation.  Returns truth_f64's dict.

    Rounding points, dg_head.hip:
      W1, W2a, W2b -> bf16           k_head_prep :82, :87, :83 (forward, fragment-major) and :89 (W2b transposed, for d hidden).
                                     Dropout2d is a zeroed weight column (wfrag :62 with the keep bits of :199-200): exact.
      features -> bf16               k_head_fwd :175 / :189; in the weight gradients k_head_wgrad3 :1217 (pack8 of the fp32 rows),
                                     k_head_wgrad2 :1058, k_head_wgrad :979; dropped channels are zeroed there (:1218, :1060, :987)
      pre-activation                 fp32 accumulator x the Dropout2d scale + b2a in fp32 (:306): nothing rounded
      hidden -> bf16                 :307, the operand of the output convolution (:322) and what is saved for the backward (:390)
      code                           s1 x accumulator + b1 + b2b + accumulator in fp32 (:378): nothing rounded
      d code -> bf16                 k_head_dh :507 / :524, k_head_dh2 :721 (the copy k_head_wgrad3 reads: :509, :724); the fp32 d code
                                     of k_head_wgrad2 / k_head_wgrad through pack8 (:1057, :979)
      d b1 = d b2b                   row sums of the fp32 d code (:507 / :721 `rs += x`, k_head_rowsum :1435): NO operand is rounded
      d hidden_pre                   bf16 W2b^T x bf16 d code in fp32, masked with hidden > 0 (:586, :625, :788)
      d b2a                          row sums of that fp32 value, before it is rounded (:587, :626, :789)
      d hidden -> bf16               :588, :627, :790: the operand of d W2a
      d W2b                          bf16 d code x bf16 hidden (k_head_dh2 :763-769; k_head_wgrad2 / k_head_wgrad on the saved hidden)
      Dropout2d scale, biases        fp32, applied to the reduced sums (k_head_reduce :1414): exact here
    Accumulation is exact here (float64); the kernels' fp32 accumulation order is what FACTOR leaves room for."""
    nl = inp.w2a is not None
    Bt, C = inp.feat.shape[:2]
    shape = inp.feat.shape
    fb = rnd(inp.feat.double()).reshape(Bt, C, -1)
    fk1 = fb * inp.keeps[0].double()[:, :, None]
    g = inp.up.double().reshape(Bt, inp.up.shape[1], -1)
    gb = rnd(g)
    w1 = rnd(inp.w1.double())
    flat = lambda t: t.permute(1, 0, 2).reshape(t.shape[1], -1)                # (Bt, R, P) -> (R, Bt P)
    out = {"pre": None}
    code = SCALE * (w1 @ fk1) + inp.b1.double()[:, None]
    out[PARAMS[0]] = SCALE * (flat(gb) @ flat(fk1).t())
    out[PARAMS[1]] = g.sum(dim=(0, 2))
    if nl:
        fk2 = fb * inp.keeps[1].double()[:, :, None]
        w2a, w2b = rnd(inp.w2a.double()), rnd(inp.w2b.double())
        pre = SCALE * (w2a @ fk2) + inp.b2a.double()[:, None]
        m = (pre > 0) if mask is None else mask.reshape(Bt, C, -1)
        hid = rnd(torch.where(m, pre, torch.zeros((), dtype=pre.dtype)))
        code = code + w2b @ hid + inp.b2b.double()[:, None]
        dhp = torch.where(m, w2b.t() @ gb, torch.zeros((), dtype=pre.dtype))
        out[PARAMS[3]] = dhp.sum(dim=(0, 2))
        out[PARAMS[2]] = SCALE * (flat(rnd(dhp)) @ flat(fk2).t())
        out[PARAMS[4]] = flat(gb) @ flat(hid).t()
        out[PARAMS[5]] = out[PARAMS[1]].clone()
        out["pre"] = pre.reshape(shape)
    out["code"] = code.reshape(Bt, -1, *shape[2:])
    return out


def bias_sum_depth(case):
    """d b1 (= d b2b) is the one gradient no operand rounding touches: the kernels sum the fp32 d code itself.  Its error is fp32
    accumulation alone, so its yardstick is the bound of that: depth x 2^-24 x sum |d code| per channel, depth = the longest chain of
    fp32 additions a term passes through.
      cluster2 present: a tile's row sum is 4 sequential additions and 4 shuffle steps (k_head_dh :507-511, k_head_dh2 :721-728), then
        k_head_reduce over the n = images x tiles partial sums (:1399-1414): ceil(n / 32) additions into one accumulator, at most 8 more
        for the remainder, 3 + 2 levels of the trees, the multiplication by the scale: ceil(n / 32) + 22.
      linear head: k_head_rowsum (:1433-1439): images x ceil(P / 256) sequential additions per thread, 8 levels of the tree."""
    Bt, P, _ = case_dims(case)
    if case.proj == "nonlinear":
        return math.ceil(Bt * ((P + 63) // 64) / 32) + 22
    return Bt * math.ceil(P / 256) + 8


def bias_sum_yardstick(case, inp, want):
    bound = bias_sum_depth(case) * 2.0 ** -24 * inp.up.double().abs().sum(dim=(0, 2, 3))
    at = int(bound.argmax())
    return {"l2": (float(bound.norm() / want.norm()), None), "elem": (float(bound.max() / want.abs().max()), (at,))}


# ---- figures --------------------------------------------------------------------------------------------------------------------
def tensor_errors(got, want, kind):
    """{figure: (value, where)} of a tensor against its reference, every figure relative as in margin_inputs.grad_errors:
        l2      ||got - want|| / ||want||
        row     weights: max over output channels of the row's ||diff|| / RMS of the reference's row norms  (where: (m,))
                code: the same over the position rows (b, y, x)
        col     weights: the same over input channels (k,)           plane   code: the same over the (b, d) planes
        elem    max |diff| / max |want|                                (where: the element's index)
    kind: "weight" (M, N) - a convolution weight (M, N, 1, 1) is taken as that -, "bias" (M,), "code" (B, D, h, w)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    if kind == "weight":
        got, want = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = got - want
    rms = lambda t: float(t.square().mean().sqrt())
    at = lambda t: tuple(int(v) for v in np.unravel_index(int(t.argmax()), t.shape))
    worst = lambda dims: (float(diff.norm(dim=dims).max()) / rms(want.norm(dim=dims)), at(diff.norm(dim=dims)))
    res = {"l2": (float(diff.norm() / want.norm()), None)}
    if kind == "weight":
        res["row"], res["col"] = worst(1), worst(0)
    elif kind == "code":
        res["row"], res["plane"] = worst(1), worst((2, 3))
    res["elem"] = (float(diff.abs().max() / want.abs().max()), at(diff.abs()))
    return {fig: res[fig] for fig in FIGURES[kind]}


def mask_report(ref, rounded):
    """From the truth's and the rounded run's pre-activations: the smallest |pre|, the largest deviation the operand rounding causes,
    the number of masks it flips, the share of the positive class, the share of (image, channel) planes inside which the mask varies."""
    pre, pre_r = ref["pre"], rounded["pre"]
    m = pre > 0
    inside = m.flatten(2).any(dim=2) & (~m).flatten(2).any(dim=2)
    return {"min_abs": float(pre.abs().min()), "deviation": float((pre_r - pre).abs().max()), "flips": int((m != (pre_r > 0)).sum()),
            "positive": float(m.double().mean()), "varying_planes": float(inside.double().mean())}


def names_of(case):
    return PARAMS[:6 if case.proj == "nonlinear" else 2] + ("code",)


Reference = namedtuple("Reference", "inp truth yard masks")


@functools.lru_cache(maxsize=None)
def case_reference(case_id):
    """(inputs, truth, {tensor: yardstick figures}, mask_report or None) of a case, computed once per process and shared; nobody
    writes into it.  The pre-activations are dropped (the largest tensors), the truth keeps code and the gradients."""
    case = case_by_id(case_id)
    inp = case_inputs(case)
    ref = truth_f64(inp)
    nl = ref["pre"] is not None
    rnd = head_manual(inp, to_bf16, mask=(ref["pre"] > 0) if nl else None)
    masks = mask_report(ref, rnd) if nl else None
    yard = {name: tensor_errors(rnd[name], ref[name], kind_of(name)) for name in names_of(case)}
    for name in (PARAMS[1], PARAMS[5]) if nl else (PARAMS[1],):
        yard[name] = bias_sum_yardstick(case, inp, ref[name])
    ref["pre"] = None
    return Reference(inp, ref, yard, masks)


def plan_of(case):
    """ops.head_plan of the case's backward (both passes of a pair in one call)."""
    from depthg_amd import ops
    Bt, P, _ = case_dims(case)
    return ops.head_plan(Bt, case.C, case.D, P)


def check_plan(case):
    """The routes and loop counts the case is about, from the library's own plan; returns the plan."""
    plan = plan_of(case)
    Bt, P, steps = case_dims(case)
    for field in ("wgrad_pair", "wgrad_single", "step_major"):
        if getattr(case, field) is not None:
            assert getattr(plan, field) == getattr(case, field), (case.id, field, plan)
    if case.dh is not None:
        assert plan.dh_route == case.dh, (case.id, plan)
        assert plan.tiles == (P + 63) // 64
    if case.loop:
        assert plan.dh_blocks > 0 and math.ceil(Bt * plan.tiles / plan.dh_blocks) >= 3, (case.id, plan)
    if case.wgrad_pair == "ONE_PASS":
        assert steps // plan.s2a >= 4, (case.id, steps, plan)
    if case.grouped is not None:
        assert steps // getattr(plan, case.grouped) >= 4, (case.id, steps, plan)
    return plan


def compare(case, got):
    """got: {tensor name: the kernels' value}.  -> (lines to print, failures): every figure against FACTOR x the yardstick's and
    the L2 cap."""
    ref = case_reference(case.id)
    lines, bad = [], []
    for name in names_of(case):
        kern = tensor_errors(got[name], ref.truth[name], kind_of(name))
        for fig, (k, where) in kern.items():
            y = ref.yard[name][fig][0]
            lines.append(f"{case.id} {name} {fig}: kernel {k:.3e} yardstick {y:.3e} ratio {k / y:.2f} (factor {FACTOR[fig]:g})"
                         + (f" at {where}" if where is not None else ""))
            if not k <= FACTOR[fig] * y or (fig == "l2" and not k <= CAP_L2):
                bad.append((name, fig, k, y, where))
    return lines, bad
