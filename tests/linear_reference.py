"""Restatement for the tests of the fused linear kernel (depthg_amd/csrc/dg_linear.hip, ops.vit_linear_forward) and of
cfg.dg_fused_linear.  Not imported by the product.

    truth       one layer - LayerNorm, linear, exact GELU, residual add as its kind configures them (src/dino/vision_transformer.py:
                49-65, 68-92, 95-115) - in float64 torch
    yardstick   the same float64 computation with the A operand (the LayerNorm output, or the input when there is no LayerNorm) and
                the weight rounded to bf16: the error no kernel with bf16 operands can avoid
    criterion   relative L2 error of the kernel against truth <= FACTOR x the yardstick's, FACTOR = 1.5 as for the attention
                (attention_reference.FACTOR).  An emulation of the prescribed arithmetic on the CPU (`emulate`: LayerNorm in fp32,
                operands rounded to bf16, fp32 matmul, fp32 bias / GELU / residual, the bf16 output rounded last) gives, at M = 257,
                Nout = 384, sigma 1 and 3 (tests/test_vit_linear_cpu.py asserts them):
                    kind            K = 128   K = 384   K = 768   K = 1536
                    ln                1.00      1.00      1.00       -        (LayerNorm needs K <= 768)
                    res               1.00      1.00      1.00      1.00
                    ln_gelu_bf16      1.20      1.21      1.22       -
                    bf16_res          1.00      1.00      1.00      1.00
                fp32 accumulation is invisible next to the operands' rounding (sqrt(K) 2^-24 against 2^-9); the one kind above 1.0 is
                the one whose OUTPUT is bf16: rounding the hidden tensor costs another 2^-9 per element on top of the operands'.
                fc2 would round that tensor anyway, so the block as a whole loses nothing; the single layer measured alone shows it.
    model       `bf16_operand_model`: a vit.VisionTransformer whose linears round input and weight to bf16 inside the fp32 torch
                formulation (optionally the attention rounds q, k, v as attention_reference's does): the whole-model yardstick.
"""
import math

import torch
import torch.nn.functional as F

from attention_reference import FACTOR, rel_l2          # noqa: F401  (re-exported: the criterion's factor is the project's one)

# kind -> (LayerNorm prologue, GELU, residual, bf16 input, bf16 output): the four launches of a block
KINDS = {"ln": (True, False, False, False, False),              # norm1 -> qkv
         "res": (False, False, True, False, False),             # proj + residual
         "ln_gelu_bf16": (True, True, False, False, True),      # norm2 -> fc1 -> GELU, handed over as bf16
         "bf16_res": (False, False, True, True, False)}         # fc2 on the bf16 hidden tensor + residual
EPS = 1e-6


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def make_case(kind, M, K, Nout, sigma=1.0, seed=0):
    """Seeded operands of one layer on the CPU.  Row 0 (and every 97th) is 100 + randn: a one-pass E[x^2] - mean^2 variance loses
    it.  x is bfloat16 for the bf16-input kind, float32 otherwise."""
    ln, _, res, in_bf16, _ = KINDS[kind]
    g = torch.Generator().manual_seed(seed)
    x = sigma * torch.randn(M, K, generator=g)
    x[::97] = 100.0 + torch.randn(x[::97].shape, generator=g)
    case = {"x": x.to(torch.bfloat16) if in_bf16 else x, "w": 0.05 * torch.randn(Nout, K, generator=g),
            "b": 0.05 * torch.randn(Nout, generator=g), "gamma": None, "beta": None, "residual": None}
    if ln:
        case["gamma"], case["beta"] = 1.0 + 0.1 * torch.randn(K, generator=g), 0.05 * torch.randn(K, generator=g)
    if res:
        case["residual"] = sigma * torch.randn(M, Nout, generator=g)
    return case


def layer_f64(kind, case, round_bf16=False):
    """Truth (round_bf16 = False) or yardstick (True) of one layer in float64, on the tensors' device."""
    ln, gelu, res, _, _ = KINDS[kind]
    a, w = case["x"].double(), case["w"].double()
    if ln:
        a = F.layer_norm(a, a.shape[-1:], case["gamma"].double(), case["beta"].double(), EPS)
    if round_bf16:
        a, w = bf16(a.float()).double(), bf16(w.float()).double()
    y = a @ w.t() + case["b"].double()
    if gelu:
        y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    if res:
        y = case["residual"].double() + y
    return y


def emulate(kind, case):
    """The prescribed arithmetic in torch: LayerNorm in fp32, operands rounded to bf16, fp32 matmul, fp32 epilogue."""
    ln, gelu, res, _, out_bf16 = KINDS[kind]
    a = case["x"].float()
    if ln:
        a = F.layer_norm(a, a.shape[-1:], case["gamma"], case["beta"], EPS)
    y = bf16(a) @ bf16(case["w"]).t() + case["b"]
    if gelu:
        y = F.gelu(y)
    if res:
        y = case["residual"] + y
    return y.to(torch.bfloat16) if out_bf16 else y


def ratios(got, kind, case):
    """(kernel error, yardstick error) against the float64 truth, both relative L2."""
    truth = layer_f64(kind, case)
    return rel_l2(got, truth), rel_l2(layer_f64(kind, case, True), truth)


def kind_fits(kind, K):
    return K <= 768 or not KINDS[kind][0]


def bf16_operand_model(model, linear=True, attention=False):
    """The whole-model yardstick: `model` (a vit.VisionTransformer, left untouched) copied with linears that round input and weight
    to bf16 and then run the fp32 torch formulation (`linear`), and / or an attention that rounds q, k, v to bf16 (`attention`)."""
    import copy
    from depthg_amd import vit
    m = copy.deepcopy(model)
    m.fused_attention = False
    m.fused_linear = False

    def rounded_linear(self, x):
        return F.linear(bf16(x), bf16(self.weight), self.bias)

    def rounded_attention(self, x, fused=False):
        p = self.qkv(x)
        y, attn, qkv = vit.attention(bf16(p), self.num_heads, self.scale)
        return self.proj(y), attn, qkv

    for blk in m.blocks:
        if linear:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                lin.forward = rounded_linear.__get__(lin)
        if attention:
            blk.attn.forward = rounded_attention.__get__(blk.attn)
    return m
