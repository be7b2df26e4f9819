// Device primitives every kernel file may use: vector types, LDS-DMA, the wave reductions, Philox, the profiling span - and
// dg_set_max_smem / dg_launch for their launchers.  Nothing here belongs to one subsystem.
#pragma once
#include "dg_common.h"
#include <map>
#include <mutex>
#include <utility>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((address_space(3))) void* lptr_t;

// LDS byte address (wave-uniform) of a pointer into the dynamic shared segment
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lptr_t)p);
}

// LDS-DMA: every lane gives its own global source address; the wave writes 64 x 16 (or 64 x 4) contiguous
// bytes at the wave-uniform LDS address.  Issued through inline asm so that hipcc neither drains it with
// vmcnt(0) before unrelated LDS reads nor counts it; completion is enforced by the explicit counted
// "s_waitcnt vmcnt" + s_barrier at the top of the tile loop (cdna guide 5.7: M0 written in the same statement).
__device__ __forceinline__ void dma16(const void* gsrc, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// ... from a wave-uniform base + a 32-bit byte offset per lane (one VGPR instead of an address pair; M0 is NOT restored: for kernels
// in which nothing else reads it)
__device__ __forceinline__ const void* dg_uniform_ptr(const void* p) {      // a wave-uniform pointer hipcc holds in VGPRs -> an SGPR pair
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const void*>(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void dma16_s(const void* sbase, uint32_t voff, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void dma4(const void* gsrc, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// a * b rounded to float32 ON ITS OWN: the empty asm hides the product from the contraction pass, so a following addition
// cannot turn the pair into one fused multiply-add (needed where a CPU reference rounds twice)
__device__ __forceinline__ float dg_mul_rn(float a, float b) {
    float r = a * b;
    asm volatile("" : "+v"(r));
    return r;
}

// ---- wave reductions.  Butterflies and DPP scans add in different orders (other bits) and cost differently: the kind is part of a kernel.
// Over the 64 lanes, result in every lane: the __shfl_xor butterfly.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// DPP row operations instead of the LDS crossbar: inclusive scan inside each row of 16 lanes (row_shr 1, 2, 4, 8), then the row
// totals carried into the odd rows (row_bcast15) - lanes 31 / 63 end up with the sums of lanes 0-31 / 32-63.
#define DG_DPP_ADD(v, ctrl, rows) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rows, 0xf, false))
#define DG_DPP_HALF_SCAN(v) DG_DPP_ADD(v, 0x111, 0xf); DG_DPP_ADD(v, 0x112, 0xf); DG_DPP_ADD(v, 0x114, 0xf); DG_DPP_ADD(v, 0x118, 0xf); DG_DPP_ADD(v, 0x142, 0xa)
// sum over the 32 lanes of each half-wave (lanes 0-31 and 32-63 separately), result in every lane of the half
__device__ __forceinline__ float half_sum(float v) {
    DG_DPP_HALF_SCAN(v);
    const float s0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
    const float s1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    return (threadIdx.x & 32) ? s1 : s0;
}
// sum over the 64 lanes, result wave-uniform
__device__ __forceinline__ float wave_sum_dpp(float v) {
    DG_DPP_HALF_SCAN(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
#undef DG_DPP_HALF_SCAN
#undef DG_DPP_ADD

// Order-preserving image of a float in the unsigned integers (larger float <-> larger key) and its inverse, for the bitwise rank
// search of dg_lhp.hip.  (dg_knn.hip's topk_key is the same mapping written with other operations: other instructions.)
__device__ __forceinline__ uint32_t dg_float_key(float x) {
    const uint32_t b = __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float dg_float_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

// dg_prof_main_span: one thread per workgroup stamps the launch's span (constant 100-MHz clock) and adds its own lifetime in
// shader cycles (s_memtime) and in wall ticks to two running sums: sum of cycles / sum of ticks = the clock the CUs HELD while
// they ran the kernel (span[2] / span[3] x 0.1 GHz).  `keep` = two 64-bit words of the workgroup's LDS (the entry stamps wait
// there: no register lives across the kernel for them).
__device__ __forceinline__ void dg_span_enter(unsigned long long* span, unsigned long long* keep) {
    if (span) {
        const unsigned long long w = (unsigned long long)wall_clock64();
        unsigned long long c;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c) :: "memory");
        keep[0] = w; keep[1] = c;
        __hip_atomic_fetch_min(&span[0], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ void dg_span_exit(unsigned long long* span, const unsigned long long* keep) {
    if (span) {
        const unsigned long long w = (unsigned long long)wall_clock64();
        unsigned long long c;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c) :: "memory");
        __hip_atomic_fetch_max(&span[1], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&span[2], c - keep[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&span[3], w - keep[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): counter (ctr, 0, 0, 0), key = the 64-bit seed
__device__ __forceinline__ uint32_t dg_philox(uint64_t seed, uint32_t ctr) {
    uint32_t c0 = ctr, c1 = 0u, c2 = 0u, c3 = 0u, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
// ... with a full 128-bit counter and all four output words (dg_philox(seed, c) == dg_philox4(seed, c, 0, 0, 0)[0])
__device__ __forceinline__ u32x4 dg_philox4(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a host round trip of a few microseconds: do it once per kernel (and
// again only if a larger size is ever needed).  Host threads of different devices may race benignly (same value).
inline hipError_t dg_set_max_smem(const void* kern, int bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, int> done;      // (kernel, device) -> bytes granted
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(kern, dev);
    auto it = done.find(key);
    if (it != done.end() && it->second >= bytes) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done[key] = bytes;
    return e;
}

// One launch: grant the kernel its dynamic LDS (`grant` false: the site's own condition says the default limit serves), launch,
// and hand back the launch's error.  A launcher that grants two kernels before it launches either, or asks for the error once
// after two launches, is not this sequence and spells its own.
template <class K, class... A>
inline hipError_t dg_launch_if(bool grant, K kern, dim3 grid, dim3 block, int smem, hipStream_t s, const A&... a) {
    if (grant) {
        const hipError_t e = dg_set_max_smem(reinterpret_cast<const void*>(kern), smem);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, block, smem, s, a...);
    return hipGetLastError();
}
template <class K, class... A>
inline hipError_t dg_launch(K kern, dim3 grid, dim3 block, int smem, hipStream_t s, const A&... a) {
    return dg_launch_if(true, kern, grid, block, smem, s, a...);
}
