// Histograms of the un-reduced code correlations (dg_corr_cd_hist): cd[b,p,q] = <x_b,p , y_b',q> of every requested pair-set is formed again
// from the operands a forward left in the workspace, binned and never stored - what the reference's training loop logs every
// cfg.hist_freq steps (src/train_segmentation.py:229-231, 298-301) without a (B,P,P) tensor reaching HBM.
//
// Two operand layouts, chosen by the plan (dg_api_corr.hip Hist):
//   Blobs  the fp16 K-major C parts of the operand blobs (already normalised) on the fp16 MFMA with fp32 accumulation - only the
//          k-steps that hold real channels, ceil(D / 16): behind a gradient pass with FOLD the padding k-step of the operand-0 blobs
//          holds the intra row means (FOLD_STASH_OFF), which this kernel therefore never touches;
//   Rows   the sampled fp32 code rows of the small sample grids on the fp32 MFMA, normalised as k_corr_small does (norm():
//          1 / max(||.||, 1e-10) per row, here applied to the finished dot product).
// Binning is torch.histc's rule over [lo, hi] - bin = floor((v - lo) nbins / (hi - lo)), v == hi into the last bin - with ONE
// difference: values outside [lo, hi] (a cosine leaves [-1, 1] by rounding only) are clamped into the end bins instead of dropped, so
// the counts of a pair-set always sum to B P P.  Padded positions (P..Ppad-1) are never counted.
// Every wave counts into a private LDS histogram (uint32, ds_add); a block adds its waves' histograms once into the int64 output with
// 64-bit integer atomics (bins the block never hit are skipped).  Integer sums do not depend on their order: the result is
// bit-reproducible, and the library's rule against floating-point atomics stands.
#include "dg_corr_args.h"

#define HIST_WAVES 4

// the 16 accumulator elements of a lane: rows (i & 3) + 8 (i >> 2) + 4 h of the streamed tile, column = the lane's stationary position
__device__ __forceinline__ void hist_count(const f32x16& v, uint32_t* wh, const float lo, const float scale, const float top,
                                           const int h, const bool col_ok, const int rows_valid) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        // (clamped as a float first: out-of-range values and NaN end in an end bin, and the conversion cannot overflow; inside the
        //  range truncation is floor)
        const float t = fminf(fmaxf((v[i] - lo) * scale, 0.f), top);
        if (col_ok && row < rows_valid) atomicAdd(&wh[(int)t], 1u);
    }
}

__device__ __forceinline__ void hist_zero(uint32_t (*hist)[DG_HIST_MAX_BINS]) {
    for (int b = threadIdx.x; b < HIST_WAVES * DG_HIST_MAX_BINS; b += 64 * HIST_WAVES) (&hist[0][0])[b] = 0u;
    __syncthreads();
}

__device__ __forceinline__ void hist_flush(const uint32_t (*hist)[DG_HIST_MAX_BINS], unsigned long long* out, const int nbins) {
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += 64 * HIST_WAVES) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < HIST_WAVES; ++w) s += hist[w][b];
        if (s) atomicAdd(out + b, (unsigned long long)s);
    }
}

// Blobs.  Block = 4 waves = 4 consecutive stationary (operand-0) tiles of one (pair-set, image); every wave keeps its tile's NK
// fragments in registers and walks the streamed operand's tiles, whose fragments it reads straight from the C parts (16 bytes per
// lane and k-step, one tile ahead; the four waves of a block read the same tiles).  NK = ceil(D / 16) k-steps.
template <int NK>
__global__ __launch_bounds__(64 * HIST_WAVES) void k_cd_hist(const DgCdHistArgs a) {
    __shared__ uint32_t hist[HIST_WAVES][DG_HIST_MAX_BINS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, r = lane & 31, h = lane >> 5;
    const int nt = a.Ppad >> 5, n = blockIdx.y, j = blockIdx.z;
    hist_zero(hist);
    const int rt = (int)blockIdx.x * HIST_WAVES + wid;
    if (rt < nt) {
        const int nS = a.sidx[j] ? (int)a.sidx[j][n] : n;
        const char* rb = a.opR + ((size_t)n * nt + rt) * a.blob_bytes + a.off_c + (h * 32 + r) * 16;
        const char* sb = a.opS[j] + (size_t)nS * nt * a.blob_bytes + a.off_c + (h * 32 + r) * 16;
        // granule 2k + h of position r: the k-th fragment of both operands
        f16x8 R[NK], A[NK], An[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            R[k] = *reinterpret_cast<const f16x8*>(rb + k * 1024);
            A[k] = *reinterpret_cast<const f16x8*>(sb + k * 1024);
        }
        const bool col_ok = rt * 32 + r < a.P;
        const float top = (float)(a.nbins - 1);
        for (int st = 0; st < nt; ++st) {
            const char* nx = sb + (size_t)(st + 1 < nt ? st + 1 : st) * a.blob_bytes;       // (past the end: a harmless re-load)
#pragma unroll
            for (int k = 0; k < NK; ++k) An[k] = *reinterpret_cast<const f16x8*>(nx + k * 1024);
            f32x16 acc = f32x16{};
#pragma unroll
            for (int k = 0; k < NK; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[k], R[k], acc, 0, 0, 0);
            hist_count(acc, hist[wid], a.lo, a.scale, top, h, col_ok, a.P - st * 32);
#pragma unroll
            for (int k = 0; k < NK; ++k) A[k] = An[k];
        }
    }
    hist_flush(hist, a.out + (size_t)j * a.nbins, a.nbins);
}

// Rows.  One wave per (streamed tile, stationary tile) pair of one (pair-set, image), the form of k_cd_mask (dg_prep.hip): lane
// (q = lane & 31, h = lane >> 5) holds the 16-byte chunks 2m + h of streamed row q (A) and of stationary row q (B); the fp32 MFMA
// pairs element e of chunk 2m with element e of chunk 2m + 1.  The squared norms come from the same registers.
template <int NC>      // 16-byte chunks of a code row per lane: D4 <= 8 NC
__global__ __launch_bounds__(64 * HIST_WAVES) void k_cd_hist_rows(const DgCdHistArgs a) {
    __shared__ uint32_t hist[HIST_WAVES][DG_HIST_MAX_BINS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, q = lane & 31, h = lane >> 5;
    const int nt = a.Ppad >> 5, D4 = a.D4, nq = D4 >> 2, n = blockIdx.y, j = blockIdx.z;
    hist_zero(hist);
    const int w = (int)blockIdx.x * HIST_WAVES + wid;
    if (w < nt * nt) {
        const int st = w / nt, rt = w - st * nt;
        const int nS = a.sidx[j] ? (int)a.sidx[j][n] : n;
        const int ps = st * 32 + q, pr = rt * 32 + q;
        const float* srow = a.rowsS[j] + ((size_t)nS * a.P + min(ps, a.P - 1)) * D4;
        const float* rrow = a.rowsR + ((size_t)n * a.P + min(pr, a.P - 1)) * D4;
        f32x4 av[NC], bv[NC];
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const int c = min(2 * m + h, nq - 1);       // (a chunk past the row: read at a clamped address and zeroed below)
            av[m] = *reinterpret_cast<const f32x4*>(srow + 4 * c);
            bv[m] = *reinterpret_cast<const f32x4*>(rrow + 4 * c);
        }
        float ss = 0.f, sr = 0.f;
#pragma unroll
        for (int m = 0; m < NC; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = 2 * m + h < nq;
                av[m][e] = in ? av[m][e] : 0.f;
                bv[m][e] = in ? bv[m][e] : 0.f;
                ss = fmaf(av[m][e], av[m][e], ss);
                sr = fmaf(bv[m][e], bv[m][e], sr);
            }
        ss += __shfl_xor(ss, 32, 64);
        sr += __shfl_xor(sr, 32, 64);
        const float invS = 1.f / fmaxf(sqrtf(ss), DG_EPS_NORM), invR = 1.f / fmaxf(sqrtf(sr), DG_EPS_NORM);
        f32x16 acc = f32x16{};
#pragma unroll
        for (int m = 0; m < NC; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][e], bv[m][e], acc, 0, 0, 0);
        // element i is (streamed row (i & 3) + 8 (i >> 2) + 4 h, stationary row q): the streamed row's factor lives in that row's lane
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = acc[i] * __shfl(invS, (i & 3) + 8 * (i >> 2) + 4 * h, 64) * invR;
        hist_count(acc, hist[wid], a.lo, a.scale, (float)(a.nbins - 1), h, pr < a.P, a.P - st * 32);
    }
    hist_flush(hist, a.out + (size_t)j * a.nbins, a.nbins);
}

hipError_t dg_launch_cd_hist(const DgCdHistArgs& a, bool rows, hipStream_t s) {
    if (a.count < 1 || a.count > DG_MAX_NEG + 2 || a.nbins < 1 || a.nbins > DG_HIST_MAX_BINS || a.P < 1 || a.Ppad % 32 || a.P > a.Ppad ||
        a.B < 1 || a.B > 65535)
        return hipErrorInvalidValue;
    const int nt = a.Ppad / 32;
    const dim3 block(64 * HIST_WAVES);
    if (rows) {
        if (a.D4 < 4 || a.D4 % 4 || a.D4 > 128) return hipErrorInvalidValue;
        const dim3 grid((nt * nt + HIST_WAVES - 1) / HIST_WAVES, a.B, a.count);
        if (a.D4 <= 72)       hipLaunchKernelGGL(k_cd_hist_rows<9>, grid, block, 0, s, a);
        else if (a.D4 <= 104) hipLaunchKernelGGL(k_cd_hist_rows<13>, grid, block, 0, s, a);
        else                  hipLaunchKernelGGL(k_cd_hist_rows<16>, grid, block, 0, s, a);
        return hipGetLastError();
    }
    const int nk = (a.D + 15) / 16;
    if (nk < 1 || nk * 16 > a.KD) return hipErrorInvalidValue;
    const dim3 grid((nt + HIST_WAVES - 1) / HIST_WAVES, a.B, a.count);
    switch (nk) {
        case 1: hipLaunchKernelGGL(k_cd_hist<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_cd_hist<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_cd_hist<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_cd_hist<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_cd_hist<5>, grid, block, 0, s, a); break;
        case 6: hipLaunchKernelGGL(k_cd_hist<6>, grid, block, 0, s, a); break;
        case 7: hipLaunchKernelGGL(k_cd_hist<7>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(k_cd_hist<8>, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}
