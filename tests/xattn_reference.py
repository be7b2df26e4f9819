"""Restatement for the tests of the fused cross-attention (depthg_amd/csrc/dg_xattn.hip, depthg_amd/cross_attn.py) and of
cfg.dg_fused_cross_attn.  Not imported by the product.

    truth       O = (softmax(q k^T * scale) * keep / (1 - p)) v and its gradients for a given d O, per (batch, head), in float64 with
                an EXPLICIT keep mask (ops.xattn_keep_mask on the GPU, any 0 / 1 tensor on the CPU)
    yardstick   the same float64 computation on q, k, v (and d O) rounded to bf16: the error no kernel with bf16 operands can avoid
    emulation   the prescribed arithmetic on the CPU: bf16 operands, fp32 scores and softmax, P (unnormalised in the forward, re-formed
                from the log-sum-exp in the backward) and dS rounded to bf16, fp32 accumulation, Di = rowsum(bf16(dO) * O)
    criterion   |x - truth| <= factor x |yardstick - truth| + floor, L2 norms over the whole tensor.
                factor, O: 1.5, the project's bound for this arithmetic (tests/attention_reference.py); the emulation at head
                    dimension 48 gives at most EMULATED_O over the grid below (tests/test_cross_attn_cpu.py asserts <= 1.2).
                factor, dQ / dK / dV: the emulation's worst ratio over the grid, EMULATED_GRAD, x 1.25 for the accumulation order.
                floor: 2^-20 x the L2 norm of the same sum with every term replaced by its magnitude - 8 float32 ulps of what the
                    accumulators hold.  It only matters where the truth cancels to nothing: with one key (or one dominant key) dS is
                    exactly 0 in float64, truth and yardstick alike, and float32 sums of the same products in two orders are not.
    figures     profiles/cross_attn_parity.md (scripts/cross_attn_parity.py writes the emulation's part)
"""
import itertools

import torch

HD = 48
FACTOR_O = 1.5
# worst ratios of the emulation over GRID (scripts/cross_attn_parity.py; random 0 / 1 masks), and what the GPU test allows
EMULATED_O = 1.138
EMULATED_GRAD = {"dq": 1.160, "dk": 1.131, "dv": 1.211}
FACTOR_GRAD = {n: 1.25 * r for n, r in EMULATED_GRAD.items()}
# the kernels on an MI355X, worst over GRID for two seeds of the exported mask (profiles/cross_attn_parity.md): O 1.139, dQ 1.158, dK 1.156, dV 1.243
FLOOR = 2.0 ** -20

SHAPES = ((1, 1), (31, 33), (33, 31), (32, 64), (65, 130), (130, 65))
BATCH_HEADS = ((1, 1), (2, 8))
PS = (0.0, 0.1, 0.5)
SIGMAS = (1.0, 3.0)
# (Nq, Nk, B, heads, p, kind): kind = a sigma, or "dominant"
GRID = [c for c in itertools.product(SHAPES, BATCH_HEADS, PS, SIGMAS)]
GRID = [(nq, nk, b, h, p, s) for ((nq, nk), (b, h), p, s) in GRID] + \
       [(nq, nk, b, h, p, "dominant") for ((nq, nk), (b, h), p) in itertools.product(((65, 130), (33, 31)), ((2, 8),), (0.0, 0.5))]


def case_id(c):
    return f"{c[0]}x{c[1]}-B{c[2]}h{c[3]}-p{c[4]}-{c[5]}"


def make_inputs(case):
    """q (B, Nq, heads * 48), k, v (B, Nk, heads * 48), d_out like q - float32 on the CPU, fixed by the case."""
    nq, nk, B, heads, p, kind = case
    g = torch.Generator().manual_seed(1000 + 7 * nq + 13 * nk + 101 * B + heads)
    sigma = 1.0 if kind == "dominant" else kind
    q = sigma * torch.randn(B, nq, heads * HD, generator=g)
    k = sigma * torch.randn(B, nk, heads * HD, generator=g)
    v = sigma * torch.randn(B, nk, heads * HD, generator=g)
    d_out = torch.randn(B, nq, heads * HD, generator=g)
    if kind == "dominant":        # every query is 43 x key j: one score of about 43 * 48 / sqrt(48) = 300 carries each row
        j = nk // 2
        q = (43.0 * k[:, j:j + 1]).expand(B, nq, heads * HD).contiguous()
    return q, k, v, d_out


def random_mask(case, seed=0):
    nq, nk, B, heads, p, _ = case
    g = torch.Generator().manual_seed(seed + 5)
    return (torch.rand(B, heads, nq, nk, generator=g) >= p).to(torch.uint8)


def heads_first(t, heads):
    B, N, C = t.shape
    return t.reshape(B, N, heads, C // heads).transpose(1, 2)


def tokens_first(t):
    B, H, N, hd = t.shape
    return t.transpose(1, 2).reshape(B, N, H * hd)


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def attention_f64(q, k, v, d_out, heads, mask, p, scale=None, round_bf16=False):
    """Truth (round_bf16 = False) or yardstick (True) -> dict(o, dq, dk, dv) float64 and, under "mag", the same four sums with every
    term replaced by its magnitude (the floor's scale)."""
    scale = HD ** -0.5 if scale is None else scale
    q, k, v, d_out = (heads_first((bf16(t) if round_bf16 else t).double(), heads) for t in (q, k, v, d_out))
    keep = mask.double() / (1.0 - p)
    P = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    Pd = P * keep
    o = Pd @ v
    dP = (d_out @ v.transpose(-1, -2)) * keep
    di = (d_out * o).sum(-1, keepdim=True)
    dS = P * (dP - di)
    res = dict(o=o, dq=scale * dS @ k, dk=scale * dS.transpose(-1, -2) @ q, dv=Pd.transpose(-1, -2) @ d_out)
    aS = P * (dP.abs() + di.abs())
    mag = dict(o=Pd @ v.abs(), dq=scale * aS @ k.abs(), dk=scale * aS.transpose(-1, -2) @ q.abs(), dv=Pd.transpose(-1, -2) @ d_out.abs())
    out = {n: tokens_first(t) for n, t in res.items()}
    out["mag"] = {n: tokens_first(t) for n, t in mag.items()}
    return out


def emulate(q, k, v, d_out, heads, mask, p, scale=None):
    """The prescribed arithmetic in float32 torch on the CPU -> dict(o, dq, dk, dv) float32."""
    scale = HD ** -0.5 if scale is None else scale
    log2e = 1.4426950408889634
    qb, kb, vb, gb = (heads_first(bf16(t.float()), heads) for t in (q, k, v, d_out))
    keep, inv_keep = mask.float(), 1.0 / (1.0 - p)
    s2 = (qb @ kb.transpose(-1, -2)) * (scale * log2e)
    m = s2.max(-1, keepdim=True).values
    pu = torch.exp2(s2 - m)
    l = pu.sum(-1, keepdim=True)
    o = (bf16(pu * keep) @ vb) * (inv_keep / l)
    lse2 = m + torch.log2(l)
    P = torch.exp2(s2 - lse2)
    dv = (bf16(P * keep).transpose(-1, -2) @ gb) * inv_keep
    di = (gb * o).sum(-1, keepdim=True)
    dS = bf16(P * ((gb @ vb.transpose(-1, -2)) * keep * inv_keep - di))
    res = dict(o=o, dq=scale * (dS @ kb), dk=scale * (dS.transpose(-1, -2) @ qb), dv=dv)
    return {n: tokens_first(t) for n, t in res.items()}


def error(got, truth):
    return float((got.double().cpu() - truth).norm())


def judge(got, truth, yard):
    """{name: (kernel error, yardstick error, floor, ratio = (kernel error - floor) / yardstick error)} - absolute L2 norms."""
    out = {}
    for n in ("o", "dq", "dk", "dv"):
        if got.get(n) is None:
            continue
        e, y, f = error(got[n], truth[n]), error(yard[n], truth[n]), FLOOR * float(truth["mag"][n].norm())
        out[n] = (e, y, f, max(e - f, 0.0) / y if y > 0 else (0.0 if e <= f else float("inf")))
    return out


def factor(name):
    return FACTOR_O if name == "o" else FACTOR_GRAD[name]


def mha_reference(mha, query, kv, mask, p):
    """`mha(query, kv, kv)[0]` of a (float64) nn.MultiheadAttention on sequence-first tokens with an explicit keep mask, in plain
    autograd-traced torch: (L, B, C) -> (L, B, C)."""
    C, H = mha.embed_dim, mha.num_heads
    w, b = mha.in_proj_weight, mha.in_proj_bias
    q = torch.nn.functional.linear(query, w[:C], b[:C]).transpose(0, 1)
    k = torch.nn.functional.linear(kv, w[C:2 * C], b[C:2 * C]).transpose(0, 1)
    v = torch.nn.functional.linear(kv, w[2 * C:], b[2 * C:]).transpose(0, 1)
    qh, kh, vh = heads_first(q, H), heads_first(k, H), heads_first(v, H)
    P = torch.softmax(qh @ kh.transpose(-1, -2) * (C // H) ** -0.5, dim=-1) * (mask.to(qh.dtype) / (1.0 - p))
    o = tokens_first(P @ vh)
    return torch.nn.functional.linear(o, mha.out_proj.weight, mha.out_proj.bias).transpose(0, 1)
