"""Inputs of the feature-cache tests (tests/test_feature_cache_cpu.py, tests/test_gpu_feature_cache.py): fp32 rows that carry the values
at which a narrowing cast can go wrong."""
import torch


def special_values():
    """fp32 values at which a narrowing cast can go wrong: infinities, NaN of both signs, fp32 and fp16 subnormals, ties (to even,
    both ways), and values that round up across a binade - for fp16 (1 + 2^-11 steps) and bf16 (1 + 2^-8 steps) - or to infinity."""
    bits = [0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
            0x00000001, 0x000116C2, 0x007FFFFF, 0x80000001,               # fp32 subnormals
            0x33800000, 0x33000000, 0x33000001, 0x337FFFFF, 0x38000000, 0x387FC000, 0x387FE000, 0x387FF000,   # fp16 subnormal range and its top
            0x3F801000, 0x3F803000, 0x3F801001, 0x3F800FFF,               # fp16 ties at 1 + 2^-11 (down to even, up to even) and beside them
            0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF,               # bf16 ties at 1 + 2^-8
            0x3FFFF000, 0x3FFFFFFF, 0x3FFF8000, 0xBFFFF000,               # round up across a binade: 1.9995 -> 2 (fp16), 1.996 -> 2 (bf16)
            0x477FE000, 0x477FF000, 0x477FEFFF, 0x47800000,               # 65504, the fp16 tie to infinity, just below it, 65536
            0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF]               # fp32 max: infinity as bf16; the bf16 tie below it
    signed = [b - (1 << 32) if b >= (1 << 31) else b for b in bits]
    return torch.tensor(signed, dtype=torch.int32).view(torch.float32)


def feature_rows(n, C, h, w, seed=0):
    """(n, C, h, w) fp32: normal draws over many binades with the special values written over the front of every row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C * h * w, generator=g) * torch.exp2(torch.randint(-20, 17, (n, C * h * w), generator=g).float())
    s = special_values()
    k = min(s.numel(), C * h * w)
    for i in range(n):
        x[i, :k] = s.roll(i)[:k]
    return x.reshape(n, C, h, w)


def exact_widen(t):
    """t.float(), bit for bit, with the NaNs widened by the IEEE rule - sign, all-ones exponent, the payload moved to the top of the
    fraction.  torch's CPU cast follows that rule for the float16 elements it converts in whole vectors of eight and stores 0x7FFFFFFF
    for a NaN among the last numel % 8 elements of a tensor (measured on torch 2.10); its device cast follows the rule everywhere.
    Everything but a NaN is widened by torch itself."""
    out = t.float().contiguous()
    if t.dtype == torch.float16:
        half = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        nan = (half & 0x7FFF) > 0x7C00
        ieee = ((half & 0x8000) << 16) | 0x7F800000 | ((half & 0x3FF) << 13)
        bits = out.view(torch.int32)
        bits[nan] = ieee.to(torch.int32)[nan]
    return out


def same_bits_or_both_nan(a, b):
    """Equal bit for bit wherever either is not a NaN, and NaN in the same places."""
    a, b = a.contiguous(), b.contiguous()
    nan = torch.isnan(a)
    return a.shape == b.shape and bool((nan == torch.isnan(b)).all()) and torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan])
