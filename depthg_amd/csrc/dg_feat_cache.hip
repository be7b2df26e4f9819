// Frozen-backbone feature cache (reference src/modules.py:90-137: `image_feat` comes out of a frozen backbone under no_grad, and
// src/train_segmentation.py:194-212 recomputes it for every batch and its positives in every epoch): (N, L) rows, L = C h w, kept as
// float32, float16 or bfloat16.
//   k_fc_put     rows idx[0..n) of the cache = src (n, L) fp32, narrowed with round-to-nearest-even (the bits of torch's .to(dtype))
//   k_fc_gather  out (2n, L) fp32 = cache rows idx_a[0..n) then idx_b[0..n), widened exactly: one launch for a batch and its positives
// Both are streams: no LDS, no atomics, every element of the rows named written once.  blockIdx.y is the row, blockIdx.x a span of
// DG_FC_SPAN cache vectors of 16 bytes (FcElem::V elements: eight 16-bit or four fp32) of it.  A row moves as whole vectors from the
// first element at which the cache row is on a 16-byte boundary, PROVIDED the fp32 row is on one there too (V * 4 bytes keep it so
// from then on): a lane then moves 16 bytes of the cache and 16 or 2 x 16 bytes of fp32 per access.  The elements in front of that
// boundary (fewer than V) and behind the last whole vector (fewer than V) go one per lane, in block 0 of the row.  Where the two
// rows never meet on a boundary (L no multiple of V, or a tensor that is not 16-byte aligned) the whole row goes one element per lane,
// still lane-contiguous.  The plan is a function of the two row addresses: uniform over the block, no divergence inside a wave.
// The row index is read from device memory (int64) by every block of the row; an index outside [0, N) ends the block before any
// address is formed from it.
#include "dg_device.h"
#include "dg_data_args.h"

template <int DT> struct FcElem;
template <> struct FcElem<DG_FC_F32> { typedef float T; static constexpr int V = 4; };
template <> struct FcElem<DG_FC_F16> { typedef _Float16 T; static constexpr int V = 8; };
template <> struct FcElem<DG_FC_BF16> { typedef uint16_t T; static constexpr int V = 8; };

// ---- one element.  fp16: v_cvt_f16_f32 / v_cvt_f32_f16 under the default mode (round to nearest even, fp16 subnormals kept).
// bf16: c10::BFloat16's round_to_nearest_even in integers (an fp32 subnormal is not flushed by a move), with the NaN pattern torch's
// vectorised CPU cast stores (at::vec cvtfp32_bf16: 0xFFFF for every NaN).
template <int DT> __device__ __forceinline__ typename FcElem<DT>::T fc_narrow(float x);
template <> __device__ __forceinline__ float fc_narrow<DG_FC_F32>(float x) { return x; }
template <> __device__ __forceinline__ _Float16 fc_narrow<DG_FC_F16>(float x) { return (_Float16)x; }
template <> __device__ __forceinline__ uint16_t fc_narrow<DG_FC_BF16>(float x) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)DG_FC_BF16_NAN;
    return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float fc_widen(float v) { return v; }
__device__ __forceinline__ float fc_widen(_Float16 v) { return (float)v; }
__device__ __forceinline__ float fc_widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

// ---- one 16-byte cache vector <-> V floats
template <int DT> struct FcVec;
template <> struct FcVec<DG_FC_F32> {
    static __device__ __forceinline__ void widen(const float* __restrict__ c, float* __restrict__ f) {
        *reinterpret_cast<f32x4*>(f) = *reinterpret_cast<const f32x4*>(c);
    }
    static __device__ __forceinline__ void narrow(const float* __restrict__ f, float* __restrict__ c) {
        *reinterpret_cast<f32x4*>(c) = *reinterpret_cast<const f32x4*>(f);
    }
};
template <> struct FcVec<DG_FC_F16> {
    static __device__ __forceinline__ void widen(const _Float16* __restrict__ c, float* __restrict__ f) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(c);
        *reinterpret_cast<f32x4*>(f) = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        *reinterpret_cast<f32x4*>(f + 4) = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
    }
    static __device__ __forceinline__ void narrow(const float* __restrict__ f, _Float16* __restrict__ c) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(f), b = *reinterpret_cast<const f32x4*>(f + 4);
        *reinterpret_cast<f16x8*>(c) = f16x8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3],
                                             (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
    }
};
template <> struct FcVec<DG_FC_BF16> {
    static __device__ __forceinline__ void widen(const uint16_t* __restrict__ c, float* __restrict__ f) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(c);          // word k: elements 2k (low half) and 2k + 1
        *reinterpret_cast<u32x4*>(f) = u32x4{v[0] << 16, v[0] & 0xffff0000u, v[1] << 16, v[1] & 0xffff0000u};
        *reinterpret_cast<u32x4*>(f + 4) = u32x4{v[2] << 16, v[2] & 0xffff0000u, v[3] << 16, v[3] & 0xffff0000u};
    }
    static __device__ __forceinline__ void narrow(const float* __restrict__ f, uint16_t* __restrict__ c) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(f), b = *reinterpret_cast<const f32x4*>(f + 4);
        u32x4 v;
        v[0] = (uint32_t)fc_narrow<DG_FC_BF16>(a[0]) | ((uint32_t)fc_narrow<DG_FC_BF16>(a[1]) << 16);
        v[1] = (uint32_t)fc_narrow<DG_FC_BF16>(a[2]) | ((uint32_t)fc_narrow<DG_FC_BF16>(a[3]) << 16);
        v[2] = (uint32_t)fc_narrow<DG_FC_BF16>(b[0]) | ((uint32_t)fc_narrow<DG_FC_BF16>(b[1]) << 16);
        v[3] = (uint32_t)fc_narrow<DG_FC_BF16>(b[2]) | ((uint32_t)fc_narrow<DG_FC_BF16>(b[3]) << 16);
        *reinterpret_cast<u32x4*>(c) = v;
    }
};

// ---- how a row moves: elements [0, head) one per lane, nvec whole vectors from element `head`, the rest one per lane
struct FcPlan { long long head, nvec; };
template <int DT> __device__ __forceinline__ FcPlan fc_plan(const void* cache_row, const float* f32_row, long long L) {
    constexpr int V = FcElem<DT>::V;
    long long head = (long long)(((16u - ((uintptr_t)cache_row & 15u)) & 15u) / sizeof(typename FcElem<DT>::T));
    if (head > L) head = L;
    if (((uintptr_t)(f32_row + head) & 15u) != 0) return FcPlan{0, 0};      // the two rows share no 16-byte boundary
    return FcPlan{head, (L - head) / V};
}

// the body both kernels share: PUT narrows f32_row into cache_row, else cache_row is widened into f32_row
template <int DT, bool PUT>
__device__ __forceinline__ void fc_move_row(typename FcElem<DT>::T* __restrict__ cache_row, float* __restrict__ f32_row, long long L) {
    constexpr int V = FcElem<DT>::V;
    const FcPlan p = fc_plan<DT>(cache_row, f32_row, L);
    auto one = [&](long long e) {
        if (PUT) cache_row[e] = fc_narrow<DT>(f32_row[e]);
        else f32_row[e] = fc_widen(cache_row[e]);
    };
    if (p.nvec == 0) {                                  // no whole vector: the row's own span of elements, lane-contiguous
        const long long e0 = (long long)blockIdx.x * (DG_FC_SPAN * V);
#pragma unroll
        for (int k = 0; k < DG_FC_UNROLL * V; ++k) {
            const long long e = e0 + k * DG_FC_THREADS + threadIdx.x;
            if (e < L) one(e);
        }
        return;
    }
    const long long v0 = (long long)blockIdx.x * DG_FC_SPAN + threadIdx.x;
#pragma unroll
    for (int u = 0; u < DG_FC_UNROLL; ++u) {            // (independent accesses: the loads of both rounds are in flight together)
        const long long v = v0 + u * DG_FC_THREADS;
        if (v < p.nvec) {
            const long long e = p.head + v * V;
            if (PUT) FcVec<DT>::narrow(f32_row + e, cache_row + e);
            else FcVec<DT>::widen(cache_row + e, f32_row + e);
        }
    }
    if (blockIdx.x == 0) {                              // fewer than V elements at either end
        if ((long long)threadIdx.x < p.head) one(threadIdx.x);
        const long long e = p.head + p.nvec * V + threadIdx.x;
        if (e < L) one(e);
    }
}

template <int DT>
__global__ __launch_bounds__(DG_FC_THREADS) void k_fc_put(typename FcElem<DT>::T* __restrict__ cache, long long N, long long L,
                                                          const float* __restrict__ src, const long long* __restrict__ idx) {
    const long long j = blockIdx.y, r = idx[j];
    if (r < 0 || r >= N) return;
    fc_move_row<DT, true>(cache + r * L, const_cast<float*>(src) + j * L, L);
}

template <int DT>
__global__ __launch_bounds__(DG_FC_THREADS) void k_fc_gather(const typename FcElem<DT>::T* __restrict__ cache, long long N, long long L,
                                                             const long long* __restrict__ idx_a, const long long* __restrict__ idx_b,
                                                             int n, float* __restrict__ out) {
    const long long j = blockIdx.y, r = j < n ? idx_a[j] : idx_b[j - n];
    if (r < 0 || r >= N) return;
    fc_move_row<DT, false>(const_cast<typename FcElem<DT>::T*>(cache) + r * L, out + j * L, L);
}

static dim3 fc_grid(long long L, int V, int rows) {
    const long long span = (long long)DG_FC_SPAN * V;
    return dim3((unsigned)((L + span - 1) / span), (unsigned)rows);
}

hipError_t dg_launch_featcache_put(void* cache, int dtype, long long N, long long L, const float* src, const long long* idx, int n,
                                   hipStream_t s) {
    const dim3 block(DG_FC_THREADS);
    if (dtype == DG_FC_F32)
        return dg_launch_if(false, k_fc_put<DG_FC_F32>, fc_grid(L, 4, n), block, 0, s, static_cast<float*>(cache), N, L, src, idx);
    if (dtype == DG_FC_F16)
        return dg_launch_if(false, k_fc_put<DG_FC_F16>, fc_grid(L, 8, n), block, 0, s, static_cast<_Float16*>(cache), N, L, src, idx);
    return dg_launch_if(false, k_fc_put<DG_FC_BF16>, fc_grid(L, 8, n), block, 0, s, static_cast<uint16_t*>(cache), N, L, src, idx);
}

hipError_t dg_launch_featcache_gather(const void* cache, int dtype, long long N, long long L, const long long* idx_a, const long long* idx_b,
                                      int n, float* out, hipStream_t s) {
    const dim3 block(DG_FC_THREADS);
    const int rows = idx_b ? 2 * n : n;
    if (dtype == DG_FC_F32)
        return dg_launch_if(false, k_fc_gather<DG_FC_F32>, fc_grid(L, 4, rows), block, 0, s, static_cast<const float*>(cache), N, L, idx_a,
                            idx_b, n, out);
    if (dtype == DG_FC_F16)
        return dg_launch_if(false, k_fc_gather<DG_FC_F16>, fc_grid(L, 8, rows), block, 0, s, static_cast<const _Float16*>(cache), N, L,
                            idx_a, idx_b, n, out);
    return dg_launch_if(false, k_fc_gather<DG_FC_BF16>, fc_grid(L, 8, rows), block, 0, s, static_cast<const uint16_t*>(cache), N, L, idx_a,
                        idx_b, n, out);
}
