"""Float64 references for the fused depth encoder (depthg_amd/csrc/dg_depth_enc.hip).  The product does not import this module.

    truth(depth, params, grad_out, residual)    float64 autograd of the nn.Sequential itself (.double(), CPU): out and the ten gradients
    chain(depth, params, grad_out, residual, rnd, out_rnd)
                                                the same chain written out by hand in float64, as the kernels walk it; with
                                                rnd = out_rnd = identity it restates `truth` (to 1e-12); with rnd = bf16 and
                                                out_rnd = fp32 it is the YARDSTICK: each operand rounded exactly where the kernels
                                                round it, everything else exact
    check(name, got, want, yard)                the criterion: |got - want| <= 1.5 x |yard - want|, in L2 and in the largest element

Rounding points of the yardstick (`rnd`, bf16 nearest-even of the fp32 value) and the kernel lines they mirror:
    W2, W3            k_de_pack: `o[j] = (__bf16)v` - the fragment images of both weights and of their transposes
    x1                de_stage1_tile: `o[j] = (__bf16)de_x1(...)` (forward, k_de_bwd_act) and de_x1_half (k_de_bwd_w2): the B operand of
                      stage 2 and of d W2
    x2                k_de_forward: the bf16x4 stores into x2l; k_de_bwd_act: `x2t[c * DG_DE_TP] = ... (__bf16)de_gelu(...)`: the B
                      operand of stage 3 and of d W3
    G (grad_out)      k_de_bwd_act: `(__bf16)de_g(...)` into the LDS tile (d x2 = G W3); k_de_bwd_w3: `a[m][ks][j] = (__bf16)de_g(...)`
                      (d W3 = G^T x2).  d b3 sums the fp32 G unrounded (in fp64).
    d a2              k_de_bwd_act: `o[j] = (__bf16)da` - to LDS (d x1 = d a2 W2) and to the workspace (d W2 = d a2^T x1).  d b2 sums
                      the fp32 value in front of the rounding.
Not rounded to bf16 anywhere: the depth map, W1 and every bias / gamma / beta, the LayerNorm statistics, n1 / n2, z1 / z2, GELU and its
derivative, d x2, d z2, d x1, d z1, d a1 (fp32 in the kernels, float64 here).  `out_rnd` (fp32) rounds what the kernels store as fp32:
the result and the ten gradients - without it d b3, which has no bf16 operand at all, would have a yardstick error of zero.
"""
import copy
import math

import torch


def identity(x):
    return x


def bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def fp32(x):
    return x.to(torch.float32).to(torch.float64)


NAMES = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3")


def make_stack(C, seed, scale=True):
    """The three-stage stack with default initial values; scale: the convolutions' weights scaled so that every stage's
    pre-norm activations are O(1) on torch.rand depth (the default initial values of a fan-in-4 convolution already are; the
    LayerNorm outputs are by construction) and the LayerNorm weights / biases moved off 1 / 0 so that their gradients matter."""
    from depthg_amd.featurizer import make_depth_downscaling
    torch.manual_seed(seed)
    stack = make_depth_downscaling(384)
    if C != 384:
        stack[6] = torch.nn.Conv2d(128, C, kernel_size=2, stride=2)
    if scale:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            stack[3].weight.mul_(4.0)
            stack[6].weight.mul_(4.0)
            for ln in (stack[1], stack[4]):
                ln.weight.add_(0.2 * torch.randn(ln.weight.shape, generator=g))
                ln.bias.add_(0.2 * torch.randn(ln.bias.shape, generator=g))
    return stack


def stack_params(stack):
    return [stack[0].weight, stack[0].bias, stack[1].weight, stack[1].bias, stack[3].weight, stack[3].bias, stack[4].weight, stack[4].bias,
            stack[6].weight, stack[6].bias]


def truth(stack, depth, grad_out, residual=None):
    """(out, [ten gradients]) by float64 autograd of a copy of the stack."""
    s = copy.deepcopy(stack).double().cpu()
    d = depth.detach().double().cpu()
    out = s(d if d.dim() == 4 else d.unsqueeze(1))
    if residual is not None:
        out = residual.detach().double().cpu() + out
    out.backward(grad_out.detach().double().cpu())
    return out.detach(), [p.grad for p in stack_params(s)]


def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _children(x):
    """(B, 2H, 2W, c) -> (B, H, W, c * 4): the 2 x 2 window under each coarser position, index c * 4 + 2 ky + kx (nn.Conv2d's order)."""
    B, H2, W2, c = x.shape
    return x.reshape(B, H2 // 2, 2, W2 // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(B, H2 // 2, W2 // 2, c * 4)


def _unchildren(x, c):
    """the inverse of _children"""
    B, H, W, _ = x.shape
    return x.reshape(B, H, W, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H, 2 * W, c)


def _ln(a, eps=1e-6):
    mu = a.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((a - mu).pow(2).mean(-1, keepdim=True) + eps)
    return (a - mu) * rstd, rstd


def _ln_back(dn, n, rstd):
    return rstd * (dn - dn.mean(-1, keepdim=True) - n * (dn * n).mean(-1, keepdim=True))


def chain(params, depth, grad_out, residual=None, rnd=identity, out_rnd=identity):
    """(out, [ten gradients]) of the stack, by hand in float64 (see the module docstring)."""
    w1, b1, g1, be1, w2, b2, g2, be2, w3, b3 = [p.detach().double().cpu() for p in params]
    C = w3.shape[0]
    d = depth.detach().double().cpu()
    d = d[:, 0] if d.dim() == 4 else d
    W1, W2, W3 = w1.reshape(64, 4), rnd(w2.reshape(128, 256)), rnd(w3.reshape(C, 512))
    d1 = _children(d.unsqueeze(-1))                              # (B, 4h, 4w, 4)
    n1, rstd1 = _ln(d1 @ W1.T + b1)
    z1 = g1 * n1 + be1
    X1 = _children(rnd(_gelu(z1)))                               # (B, 2h, 2w, 256)
    n2, rstd2 = _ln(X1 @ W2.T + b2)
    z2 = g2 * n2 + be2
    X2 = _children(rnd(_gelu(z2)))                               # (B, h, w, 512)
    out = (X2 @ W3.T + b3).permute(0, 3, 1, 2)
    if residual is not None:
        out = residual.detach().double().cpu() + out
    G = grad_out.detach().double().cpu().permute(0, 2, 3, 1)      # (B, h, w, C)
    Gr = rnd(G)
    dW3 = torch.einsum("bhwc,bhwk->ck", Gr, X2).reshape(C, 128, 2, 2)
    db3 = G.sum((0, 1, 2))
    dz2 = _unchildren(Gr @ W3, 128) * _gelu_grad(z2)
    dg2, dbe2 = (dz2 * n2).sum((0, 1, 2)), dz2.sum((0, 1, 2))
    da2 = _ln_back(dz2 * g2, n2, rstd2)
    db2 = da2.sum((0, 1, 2))
    da2r = rnd(da2)
    dW2 = torch.einsum("bhwc,bhwk->ck", da2r, X1).reshape(128, 64, 2, 2)
    dz1 = _unchildren(da2r @ W2, 64) * _gelu_grad(z1)
    dg1, dbe1 = (dz1 * n1).sum((0, 1, 2)), dz1.sum((0, 1, 2))
    da1 = _ln_back(dz1 * g1, n1, rstd1)
    db1 = da1.sum((0, 1, 2))
    dW1 = torch.einsum("bhwc,bhwk->ck", da1, d1).reshape(64, 1, 2, 2)
    grads = [dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dW3, db3]
    return out_rnd(out), [out_rnd(g) for g in grads]


def yardstick(params, depth, grad_out, residual=None):
    return chain(params, depth, grad_out, residual, rnd=bf16, out_rnd=fp32)


FACTOR = 1.5          # the factor tests/test_gpu_attention.py and tests/test_gpu_vit_linear.py hold for the bf16 MFMA paths


def errors(got, want, yard):
    """(kernel L2, yardstick L2, kernel max, yardstick max) of one tensor against the truth (absolute: a gradient that is exactly
    zero - d W1 on a zero depth map - has no relative error, and 0 <= 1.5 x 0 holds)."""
    got, want, yard = got.detach().double().cpu(), want.double(), yard.double()
    return (float((got - want).norm()), float((yard - want).norm()), float((got - want).abs().max()), float((yard - want).abs().max()))


def check(name, got, want, yard, log=None):
    kl2, yl2, kmax, ymax = errors(got, want, yard)
    scale = float(want.norm()) or 1.0
    line = f"{name}: L2 kernel {kl2 / scale:.3e} yardstick {yl2 / scale:.3e} ratio {kl2 / yl2 if yl2 else float(kl2 > 0):.3f}; " \
           f"max kernel {kmax:.3e} yardstick {ymax:.3e} ratio {kmax / ymax if ymax else float(kmax > 0):.3f}"
    print(line)
    if log is not None:
        log.append(line)
    assert bool(torch.isfinite(got).all()), name
    assert kl2 <= FACTOR * yl2, line
    assert kmax <= FACTOR * ymax, line
