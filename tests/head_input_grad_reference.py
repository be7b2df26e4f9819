"""Reference and yardstick for d loss / d image_feat of the projection head (tests/test_gpu_head_input_grad.py,
tests/test_depth_featurizer_cpu.py).  Not imported by the product.

    dx[b,k,p] = s keep1[b,k] sum_d W1[d,k] g[b,d,p] + s keep2[b,k] sum_j W2a[j,k] dh[b,j,p]      (second term: nonlinear head)
    dh[b,j,p] = [hidden[b,j,p] > 0] sum_d W2b[d,j] g[b,d,p]
with g = d code, s = 1 / (1 - p) where the keep mask exists (else keep = 1, s = 1).

    cases       every case of tests/head_margin_inputs.py (its inputs flip no ReLU mask) and two small ones of this module: an
                eval-mode head without keep masks, and a pair in which only the second pass requires grad.
    truth       float64 autograd of oracle.head_oracle.head_forward with respect to the features (dx_truth).
    yardstick   dx_manual: the same products in float64 with each operand rounded to bf16 where the kernels round it, mask the
                truth's.  Rounding points (depthg_amd/csrc/dg_head.hip):
                  W1, W2a -> bf16      k_head_dx_prep `out[i] = (__bf16)v` (the transposed fragment-major copies)
                  d code -> bf16       k_head_dx, the g tile: `o[e] = (__bf16)(ok ? v[e] : 0.f)` / the guarded form below it
                  W2b -> bf16          k_head_prep :89 (W2b transposed, for d hidden)
                  d hidden -> bf16     k_head_dh :588, :627, k_head_dh2 :790 - bf16 W2b^T x bf16 d code in fp32, masked, rounded;
                                       k_head_dx reads those bf16 values as they are
                  Dropout2d            a zeroed weight column (`wfrag(wc[j], mk ...)`): exact; the scale multiplies the fp32
                                       accumulator in the epilogue (`acc[i][j] * sfin`): nothing rounded
    figures     head_margin_inputs.tensor_errors(..., "code"); criterion: FACTOR x the yardstick's, CAP_L2 - that module's.
"""
import functools
from collections import namedtuple

import torch

import head_margin_inputs as H
from oracle import head_oracle as HO

# the two small cases: (B, C, D, hw) = (3, 64, 16, 3) in eval mode, (2, 64, 16, 3) as a pair whose first pass does not require grad
SMALL_EVAL = H.Case("small-eval-no-keeps", False, 3, 64, 16, 3, "nonlinear", 21, "TILES", None, None, False, False, None,
                    "eval mode: no keep masks, no scale; P = 9 on every guarded path")
SMALL_PAIR = H.Case("small-pair-second-only", True, 2, 64, 16, 3, "nonlinear", 22, "TILES", None, None, False, False, None,
                    "pair: only image_feat_pos requires grad - the launch walks images B.. alone")
CASES = list(H.CASES) + [SMALL_EVAL, SMALL_PAIR]


def case_inputs(case):
    """head_margin_inputs' inputs; the eval case has keeps None and b2a placed for the unscaled, undropped pre-activation."""
    if case.id != SMALL_EVAL.id:
        return H.case_inputs(case)
    Bt, P, _ = H.case_dims(case)
    C, D, hw = case.C, case.D, case.hw
    g = torch.Generator().manual_seed(4000 + case.seed)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    proto = rn(H.PROTOTYPES, C) * 2.0
    pick = torch.randint(0, H.PROTOTYPES, (Bt, P), generator=g)
    feat = (proto[pick] + H.NOISE * rn(Bt, P, C)).permute(0, 2, 1).reshape(Bt, C, hw, hw).contiguous().float()
    # (all channels kept in every pattern; _margin_w2a works with SCALE x the products, eval mode has no scale)
    w2a, b2a = H._margin_w2a(proto, torch.ones(H.PATTERNS, C, dtype=torch.float64), C, g)
    b2a = (b2a.double() / H.SCALE).float()
    w1, w2b = (rn(D, C) / C ** 0.5).float(), (rn(D, C) / C ** 0.5).float()
    b1, b2b = (0.1 * rn(D)).float(), (0.1 * rn(D)).float()
    return H.Inputs(feat, None, w1, b1, w2a, b2a, w2b, b2b, rn(Bt, D, hw, hw).float())


def _keep_factor(keeps, i, like):
    """s keep_i as (Bt, C, 1), or ones where the draw does not exist"""
    if keeps is None or keeps[i] is None:
        return torch.ones(like.shape[0], like.shape[1], 1, dtype=torch.float64)
    return (keeps[i].double() * H.SCALE)[:, :, None]


def pre_activation(inp):
    """cluster2's pre-activation in float64 (Bt, C, P), None for the linear head"""
    if inp.w2a is None:
        return None
    f = inp.feat.double().flatten(2)
    return inp.w2a.double() @ (f * _keep_factor(inp.keeps, 1, f)) + inp.b2a.double()[:, None]


def dx_truth(inp):
    """float64 autograd of oracle.head_oracle.head_forward with respect to the features, upstream `up` on code -> (Bt, C, hw, hw)"""
    nl = inp.w2a is not None
    prm = [t.double() for t in (inp.w1, inp.b1) + ((inp.w2a, inp.b2a, inp.w2b, inp.b2b) if nl else ())]
    f = inp.feat.double().requires_grad_(True)
    keeps = None if inp.keeps is None else tuple(k.double() for k in inp.keeps)
    code, _ = HO.head_forward(f, *prm, keeps=keeps, p=H.P_DROP)
    (code * inp.up.double()).sum().backward()
    return f.grad


def dx_manual(inp, rnd, mask=None):
    """The formula of the module docstring in float64, `rnd` on every operand the kernels round (identity restates the truth).
    mask: the ReLU mask (Bt, C, P) or None for this run's own pre-activation's."""
    shape = inp.feat.shape
    g = rnd(inp.up.double().flatten(2))
    dx = _keep_factor(inp.keeps, 0, inp.feat) * (rnd(inp.w1.double()).t() @ g)
    if inp.w2a is not None:
        if mask is None:
            mask = pre_activation(inp) > 0
        dh = rnd(torch.where(mask, rnd(inp.w2b.double()).t() @ g, torch.zeros((), dtype=torch.float64)))
        dx = dx + _keep_factor(inp.keeps, 1, inp.feat) * (rnd(inp.w2a.double()).t() @ dh)
    return dx.reshape(shape)


Reference = namedtuple("Reference", "inp truth yard")


@functools.lru_cache(maxsize=None)
def case_reference(case_id):
    """(inputs, float64 dx, the yardstick's figures) of a case, computed once per process and shared; nobody writes into it."""
    case = next(k for k in CASES if k.id == case_id)
    inp = case_inputs(case)
    truth = dx_truth(inp)
    pre = pre_activation(inp)
    rounded = dx_manual(inp, H.to_bf16, mask=None if pre is None else pre > 0)
    return Reference(inp, truth, H.tensor_errors(rounded, truth, "code"))


def compare(case, got, images=slice(None)):
    """got: the kernels' dx of the images `images` of the case.  -> (lines to print, failures) by head_margin_inputs' criterion:
    every figure <= FACTOR x the yardstick's (the yardstick taken over the same images), every L2 <= CAP_L2."""
    ref = case_reference(case.id)
    yard = ref.yard
    if images != slice(None):
        pre = pre_activation(ref.inp)
        rounded = dx_manual(ref.inp, H.to_bf16, mask=None if pre is None else pre > 0)
        yard = H.tensor_errors(rounded[images], ref.truth[images], "code")
    lines, bad = [], []
    for fig, (k, where) in H.tensor_errors(got, ref.truth[images], "code").items():
        y = yard[fig][0]
        lines.append(f"{case.id} d image_feat {fig}: kernel {k:.3e} yardstick {y:.3e} ratio {k / y:.2f} (factor {H.FACTOR[fig]:g})"
                     + (f" at {where}" if where is not None else ""))
        if not k <= H.FACTOR[fig] * y or (fig == "l2" and not k <= H.CAP_L2):
            bad.append((fig, k, y, where))
    return lines, bad
