// The three-stage depth encoder of DinoFeaturizerWithDepth (src/modules.py:497-506 the stack, :557 its call, :562-563 the "sum"
// guidance, :619-631 LayerNorm2d) as fused kernels, forward and backward:
//     Conv2d(1,64,2,2), LayerNorm2d(64), GELU, Conv2d(64,128,2,2), LayerNorm2d(128), GELU, Conv2d(128,C,2,2)   [+ residual]
// The convolutions have stride = kernel, so an output position (b, y, x) depends on the 8 x 8 depth patch at (8y, 8x) alone: 16
// stage-1 sub-positions s1 = 4 s2 + q (s2 = the 2 x 2 stage-2 sub-position (sy, sx) the sub-position feeds, q = its place (qy, qx)
// in that one's 2 x 2 window) and 4 stage-2 sub-positions.  With the reductions ordered k2 = 64 q + c1 and k3 = 128 s2 + c2,
//     stage 2 is X2 (4 N x 128) = X1 (4 N x 256) W2^T,   stage 3 is OUT (N x C) = X2 (N x 512) W3^T,     N = B h w positions,
// and a row of either left operand is contiguous in the tile a workgroup holds.  Tiles of DG_DE_TP = 32 positions, 4 waves.
// Stage 1 (K = 4) runs on the VALU in fp32; stages 2 and 3 and the four products of the backward run on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation: lane (r, h) = (lane & 31, lane >> 5) gives A[row r][k = 8 h + j] and
// B[column r][k = 8 h + j], accumulator element i of the lane is row de_row(i, h), column r (dg_linear.hip).  The weights are the
// A operands, read from bf16 fragment-order copies the launch itself makes in the workspace (k_de_pack); a position sits on a lane.
// LayerNorm statistics (biased variance, eps inside the root), normalisation, exact GELU and the biases are fp32.
//   k_de_pack      W2, W3 (and for the backward their transposes) -> bf16 fragment images
//   k_de_forward   one block per tile: stage 1 -> LDS (bf16), stage 2 (wave w = sub-position s2) -> LDS (bf16), stage 3 (the waves
//                  share the C / 32 channel tiles) + b3 + residual -> out; nothing else reaches global memory
//   k_de_bwd_act   blocks walk the tiles blockIdx, blockIdx + grid, ...: stages 1 and 2 re-formed from the depth map, x2 (bf16) to the
//                  workspace; d x2 = G W3 from the upstream gradient (bf16 in LDS), back through GELU and LayerNorm 2 to d a2 (bf16
//                  to the workspace and to LDS), d x1 = d a2 W2, back through GELU and LayerNorm 1 in the accumulators' own layout;
//                  the gradients of W1, b1, gamma1, beta1, b2, gamma2, beta2 summed per lane half (DPP), per wave, per block
//                  (LDS, fixed order) through the block's tiles: one partial vector of DG_DE_SP floats per block
//   k_de_bwd_w2    grid (child q, split): d W2[:, :, q] += d a2^T x1(q) over the split's tiles, x1 of that child re-formed from the
//                  depth map (nothing of stage-1 size is ever stored), accumulators live through the tiles
//   k_de_bwd_w3    grid (chunk of 64 channels, split): d W3 += G^T x2 with both operands straight from global memory in fragment
//                  order (G is (B, C, h, w): positions are contiguous), d b3 from the fp32 G in fp64
//   k_de_combine   partials -> gradients, fp64, fixed order; every element written
// bf16 rounding points (tests/depth_encoder_reference.py mirrors them): W2, W3 (k_de_pack), x1 (de_stage1_tile / k_de_bwd_w2), x2
// (k_de_forward, k_de_bwd_act), the upstream gradient G (k_de_bwd_act's LDS tile, k_de_bwd_w3's A operand), d a2 (k_de_bwd_act).
// No atomics: every result is a function of the inputs alone, bit for bit.
#include "dg_depth_args.h"
#include "dg_device.h"
#include <cstring>

#define DE_THREADS 256
#define DE_EPS 1e-6f
#define DE_X1_PITCH 528                  // bytes per row of the stage-1 tile (256 bf16 + 16: conflict-free 128-bit fragment reads)
#define DE_X2_PITCH 1040                 // ... of the stage-2 tile (512 bf16 + 16)
#define DE_DA_PITCH 272                  // ... of a row of 128 bf16 (+ 16)
#define DE_RSQRT2 0.70710678118654752440f
#define DE_RSQRT2PI 0.39894228040143267794f

static_assert(DG_DE_TP == 32 && DE_THREADS == 256, "four waves; a tile's positions are the 32 columns of an MFMA");

__device__ __forceinline__ int de_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }      // accumulator element -> tile row
__device__ __forceinline__ float de_gelu(float z) { return 0.5f * z * (1.f + erff(z * DE_RSQRT2)); }
__device__ __forceinline__ float de_gelu_grad(float z) {
    return 0.5f * (1.f + erff(z * DE_RSQRT2)) + z * DE_RSQRT2PI * expf(-0.5f * z * z);
}
#define DE_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

// ---- the weights' bf16 fragment images: per (tile of 32 rows, k-step of 16) 64 lanes x 8 values, lane (r, h) = M[32 t + r][16 ks + 8 h + j]
//   pack_w2  M = W2  rows c2, k = 64 q + c1          pack_w2t  M = W2^T rows k2 = 64 q + c1, k = c2
//   pack_w3  M = W3  rows c,  k = 128 s2 + c2        pack_w3t  M = W3^T rows k3 = 128 s2 + c2, k = c
// (nn.Conv2d stores W2 as [c2][c1][q] and W3 as [c][c2][s2].)  One thread per 16-byte piece.
__global__ __launch_bounds__(DE_THREADS) void k_de_pack(const DgDepthEncArgs A, int with_t) {
    const size_t n2 = (size_t)DG_DE_C2 * DG_DE_K2 / 8, n3 = (size_t)A.C * DG_DE_K3 / 8;
    size_t e = (size_t)blockIdx.x * DE_THREADS + threadIdx.x;
    int mode;
    bf16x8* dst;
    if (e < n2) { mode = 0; dst = static_cast<bf16x8*>(A.pack_w2); }
    else if ((e -= n2) < n3) { mode = 2; dst = static_cast<bf16x8*>(A.pack_w3); }
    else if (!with_t) return;
    else if ((e -= n3) < n2) { mode = 1; dst = static_cast<bf16x8*>(A.pack_w2t); }
    else if ((e -= n2) < n3) { mode = 3; dst = static_cast<bf16x8*>(A.pack_w3t); }
    else return;
    const int lane = (int)(e & 63), r = lane & 31, h = lane >> 5;
    const int KS = mode == 0 ? 16 : mode == 2 ? 32 : mode == 1 ? 8 : A.C / 16;
    const int f = (int)(e >> 6), ks = f % KS, t = f / KS, row = 32 * t + r, k0 = 16 * ks + 8 * h;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        float v;
        if (mode == 0) v = A.w2[row * 256 + (k & 63) * 4 + (k >> 6)];
        else if (mode == 1) v = A.w2[k * 256 + (row & 63) * 4 + (row >> 6)];
        else if (mode == 2) v = A.w3[(size_t)row * 512 + (k & 127) * 4 + (k >> 7)];
        else v = A.w3[(size_t)k * 512 + (row & 127) * 4 + (row >> 7)];
        o[j] = (__bf16)v;
    }
    dst[e] = o;
}

// ---- what the kernels share
// The small parameters in LDS, in the order of the partial vector (dg_depth_args.h): W1, b1, gamma1, beta1, b2, gamma2, beta2.
__device__ __forceinline__ void de_load_params(const DgDepthEncArgs& A, float* pl, bool stage2) {
    for (int i = threadIdx.x; i < DG_DE_SP; i += DE_THREADS) {
        float v = 0.f;
        if (i < DG_DE_SP_B1) v = A.w1[i];
        else if (i < DG_DE_SP_G1) v = A.b1[i - DG_DE_SP_B1];
        else if (i < DG_DE_SP_BE1) v = A.g1[i - DG_DE_SP_G1];
        else if (i < DG_DE_SP_B2) v = A.be1[i - DG_DE_SP_BE1];
        else if (!stage2) break;
        else if (i < DG_DE_SP_G2) v = A.b2[i - DG_DE_SP_B2];
        else if (i < DG_DE_SP_BE2) v = A.g2[i - DG_DE_SP_G2];
        else v = A.be2[i - DG_DE_SP_BE2];
        pl[i] = v;
    }
}

// the four depth values under stage-1 sub-position s1 of position n (0 past the last position)
__device__ __forceinline__ void de_load_depth(const DgDepthEncArgs& A, int n, int s1, float (&d)[4]) {
    d[0] = d[1] = d[2] = d[3] = 0.f;
    if (n >= A.N) return;
    const int b = n / A.P, p = n - b * A.P, y = p / A.w, x = p - y * A.w;
    const int s2 = s1 >> 2, q = s1 & 3, Y1 = 2 * (s2 >> 1) + (q >> 1), X1 = 2 * (s2 & 1) + (q & 1);
    const size_t dw = (size_t)8 * A.w;
    const float* src = A.depth + ((size_t)b * 8 * A.h + 8 * y + 2 * Y1) * dw + 8 * x + 2 * X1;
    d[0] = src[0]; d[1] = src[1]; d[2] = src[dw]; d[3] = src[dw + 1];
}

// stage 1 of one sub-position: a1 of channel c (the same chain wherever it is formed again: the same bits)
__device__ __forceinline__ float de_a1(const float* pl, const float (&d)[4], int c) {
    const float* w = pl + 4 * c;
    return fmaf(w[3], d[3], fmaf(w[2], d[2], fmaf(w[1], d[1], fmaf(w[0], d[0], pl[DG_DE_SP_B1 + c]))));
}
__device__ __forceinline__ void de_s1_stats(const float* pl, const float (&d)[4], float& mu, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DG_DE_C1; ++c) s += de_a1(pl, d, c);
    mu = s * (1.f / DG_DE_C1);
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < DG_DE_C1; ++c) { const float v = de_a1(pl, d, c) - mu; q = fmaf(v, v, q); }
    rstd = 1.f / sqrtf(q * (1.f / DG_DE_C1) + DE_EPS);
}
__device__ __forceinline__ float de_x1(const float* pl, const float (&d)[4], float mu, float rstd, int c) {
    return de_gelu(fmaf(pl[DG_DE_SP_G1 + c], (de_a1(pl, d, c) - mu) * rstd, pl[DG_DE_SP_BE1 + c]));
}

// Stage 1 of a tile -> x1l[row 32 s2 + pos][64 q + c1] (bf16).  A thread takes the sub-positions s1 = thread >> 5 and + 8 of position
// thread & 31.  dl / st (or null): the depth values [32 s1 + pos][4] and the statistics [32 s1 + pos][2] for the backward.
__device__ __forceinline__ void de_stage1_tile(const DgDepthEncArgs& A, const float* pl, int n0, uint8_t* x1l, float* dl, float* st) {
    const int pos = threadIdx.x & 31;
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
        const int s1 = it * 8 + (threadIdx.x >> 5), s2 = s1 >> 2, q = s1 & 3;
        float d[4], mu, rstd;
        de_load_depth(A, n0 + pos, s1, d);
        de_s1_stats(pl, d, mu, rstd);
        uint8_t* dst = x1l + (size_t)(32 * s2 + pos) * DE_X1_PITCH + 128 * q;
#pragma unroll
        for (int c0 = 0; c0 < DG_DE_C1; c0 += 8) {
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (__bf16)de_x1(pl, d, mu, rstd, c0 + j);
            *reinterpret_cast<bf16x8*>(dst + 2 * c0) = o;
        }
        if (dl) {
            const int row = 32 * s1 + pos;
            *reinterpret_cast<f32x4*>(dl + 4 * row) = f32x4{d[0], d[1], d[2], d[3]};
            st[2 * row] = mu; st[2 * row + 1] = rstd;
        }
    }
}

// Stage 2 of the wave's sub-position s2 = wave for the tile's 32 positions: acc[t][i] = n2 (normalised, in front of gamma2 / beta2)
// of channel 32 t + de_row(i, h) at position r; returns rstd.
__device__ __forceinline__ float de_stage2(const DgDepthEncArgs& A, const float* pl, const uint8_t* x1l, int wave, int lane, f32x16 (&acc)[4]) {
    const int r = lane & 31, h = lane >> 5;
    const bf16x8* wp = static_cast<const bf16x8*>(A.pack_w2) + lane;
    const uint8_t* xb = x1l + (size_t)(32 * wave + r) * DE_X1_PITCH + 16 * h;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
#pragma unroll 4
    for (int ks = 0; ks < DG_DE_K2 / 16; ++ks) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(xb + 32 * ks);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = DE_MFMA(wp[(t * (DG_DE_K2 / 16) + ks) * 64], b, acc[t]);
    }
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[t][i] += pl[DG_DE_SP_B2 + 32 * t + de_row(i, h)]; s += acc[t][i]; }
    s += __shfl_xor(s, 32, 64);
    const float mu = s * (1.f / DG_DE_C2);
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[t][i] -= mu; q = fmaf(acc[t][i], acc[t][i], q); }
    q += __shfl_xor(q, 32, 64);
    const float rstd = 1.f / sqrtf(q * (1.f / DG_DE_C2) + DE_EPS);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] *= rstd;
    return rstd;
}
__device__ __forceinline__ float de_z2(const float* pl, float n2, int c) { return fmaf(pl[DG_DE_SP_G2 + c], n2, pl[DG_DE_SP_BE2 + c]); }

// G[position n0 + i][channel c] of the (B, C, h, w) upstream gradient; 0 past the last position.  (b0, p0): image and offset of n0.
__device__ __forceinline__ float de_g(const DgDepthEncArgs& A, int n0, int b0, int p0, int i, int c) {
    if (n0 + i >= A.N) return 0.f;
    int p = p0 + i, b = b0;
    if (p >= A.P) { const int k = p / A.P; b += k; p -= k * A.P; }
    return A.grad_out[((size_t)b * A.C + c) * A.P + p];
}

// ---- forward.  grid tiles, block 256, dynamic LDS de_fwd_lds().
static constexpr int de_fwd_lds() { return 128 * DE_X1_PITCH + DG_DE_TP * DE_X2_PITCH + DG_DE_SP * 4; }
__global__ __launch_bounds__(DE_THREADS) void k_de_forward(const DgDepthEncArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t de_lds[];
    uint8_t* x1l = de_lds;
    uint8_t* x2l = x1l + 128 * DE_X1_PITCH;
    float* pl = reinterpret_cast<float*>(x2l + DG_DE_TP * DE_X2_PITCH);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * DG_DE_TP;
    de_load_params(A, pl, true);
    __syncthreads();
    de_stage1_tile(A, pl, n0, x1l, nullptr, nullptr);
    __syncthreads();
    {
        f32x16 acc[4];
        de_stage2(A, pl, x1l, wave, lane, acc);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (__bf16)de_gelu(de_z2(pl, acc[t][4 * g + j], 32 * t + 8 * g + 4 * h + j));
                *reinterpret_cast<bf16x4*>(x2l + (size_t)r * DE_X2_PITCH + 2 * (128 * wave + 32 * t + 8 * g + 4 * h)) = o;
            }
    }
    __syncthreads();
    const int n = n0 + r;
    const bool ok = n < A.N;
    const int b = ok ? n / A.P : 0, p = ok ? n - b * A.P : 0;
    const uint8_t* xb = x2l + (size_t)r * DE_X2_PITCH + 16 * h;
    for (int t = wave; t < A.C / 32; t += 4) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        const bf16x8* wp = static_cast<const bf16x8*>(A.pack_w3) + (size_t)t * (DG_DE_K3 / 16) * 64 + lane;
#pragma unroll 8
        for (int ks = 0; ks < DG_DE_K3 / 16; ++ks) acc = DE_MFMA(wp[ks * 64], *reinterpret_cast<const bf16x8*>(xb + 32 * ks), acc);
        if (ok) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = 32 * t + de_row(i, h);
                const size_t o = ((size_t)b * A.C + c) * A.P + p;
                float v = acc[i] + A.b3[c];
                if (A.residual) v = A.residual[o] + v;
                A.out[o] = v;
            }
        }
    }
}

// ---- backward: the activation gradients and the small parameters' partial sums.  grid blocks_act, block 256, LDS de_act_lds(C).
static inline int de_act_lds(int C) {
    return 128 * DE_X1_PITCH + DG_DE_TP * (2 * C + 16) + 512 * 4 * 4 + 512 * 2 * 4 + DG_DE_SP * 4 * 6;
}
__global__ __launch_bounds__(DE_THREADS) void k_de_bwd_act(const DgDepthEncArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t de_lds[];
    const int gp = 2 * A.C + 16;                                  // bytes per row of the upstream gradient's tile
    uint8_t* x1l = de_lds;                                        // stage-1 tile; later the wave's own rows hold d a2 [row][128]
    uint8_t* gl = x1l + 128 * DE_X1_PITCH;                        // G [pos][C] bf16
    float* dl = reinterpret_cast<float*>(gl + DG_DE_TP * gp);     // depth values [32 s1 + pos][4]
    float* st = dl + 512 * 4;                                     // stage-1 statistics [32 s1 + pos][2]
    float* pl = st + 512 * 2;                                     // parameters
    float* red = pl + DG_DE_SP;                                   // [wave][DG_DE_SP]: the tile's sums per wave
    float* accl = red + 4 * DG_DE_SP;                             // the block's sums through its tiles
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31, h = lane >> 5;
    de_load_params(A, pl, true);
    for (int i = threadIdx.x; i < DG_DE_SP; i += DE_THREADS) accl[i] = 0.f;
    __syncthreads();
    float* redw = red + wave * DG_DE_SP;
    for (int tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const int n0 = tile * DG_DE_TP, b0 = n0 / A.P, p0 = n0 - b0 * A.P;
        const bool ok = n0 + r < A.N;
        de_stage1_tile(A, pl, n0, x1l, dl, st);
        for (int idx = threadIdx.x; idx < A.C * DG_DE_TP; idx += DE_THREADS) {
            const int c = idx >> 5, i = idx & 31;
            *reinterpret_cast<__bf16*>(gl + (size_t)i * gp + 2 * c) = (__bf16)de_g(A, n0, b0, p0, i, c);
        }
        __syncthreads();
        f32x16 n2[4], dx[4];
        const float rstd2 = de_stage2(A, pl, x1l, wave, lane, n2);
        {   // x2 -> workspace [tile][128 s2 + c2][pos]; zero past the last position
            __bf16* x2t = static_cast<__bf16*>(A.x2t) + ((size_t)tile * DG_DE_K3 + 128 * wave) * DG_DE_TP + r;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = 32 * t + de_row(i, h);
                    x2t[c * DG_DE_TP] = ok ? (__bf16)de_gelu(de_z2(pl, n2[t][i], c)) : (__bf16)0.f;
                }
        }
        {   // d x2^T (rows 128 wave + c2, the tile's positions) = W3^T G^T
            const int KS = A.C / 16;
            const bf16x8* wp = static_cast<const bf16x8*>(A.pack_w3t) + (size_t)(4 * wave) * KS * 64 + lane;
            const uint8_t* gb = gl + (size_t)r * gp + 16 * h;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) dx[t][i] = 0.f;
#pragma unroll 2
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(gb + 32 * ks);
#pragma unroll
                for (int t = 0; t < 4; ++t) dx[t] = DE_MFMA(wp[((size_t)t * KS + ks) * 64], b, dx[t]);
            }
        }
        {   // through GELU and LayerNorm 2: dx <- d a2; the sums of d beta2, d gamma2, d b2 over the wave's 32 positions
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = 32 * t + de_row(i, h);
                    const float n = n2[t][i], dz = dx[t][i] * de_gelu_grad(de_z2(pl, n, c));
                    const float sb = half_sum(dz), sg = half_sum(dz * n);
                    if (r == 0) { redw[DG_DE_SP_BE2 + c] = sb; redw[DG_DE_SP_G2 + c] = sg; }
                    const float dn = dz * pl[DG_DE_SP_G2 + c];
                    dx[t][i] = dn; s1 += dn; s2 = fmaf(dn, n, s2);
                }
            s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            const float m1 = s1 * (1.f / DG_DE_C2), m2 = s2 * (1.f / DG_DE_C2);
            __bf16* dat = static_cast<__bf16*>(A.da2t) + (size_t)tile * DG_DE_C2 * 128 + 32 * wave + r;
            uint8_t* dal = x1l + (size_t)(32 * wave + r) * DE_X1_PITCH;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bf16x4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = 4 * g + j, c = 32 * t + 8 * g + 4 * h + j;
                        const float da = rstd2 * (dx[t][i] - m1 - n2[t][i] * m2);
                        const float sb = half_sum(da);
                        if (r == 0) redw[DG_DE_SP_B2 + c] = sb;
                        o[j] = (__bf16)da;
                        dat[(size_t)c * 128] = o[j];
                    }
                    *reinterpret_cast<bf16x4*>(dal + 2 * (32 * t + 8 * g + 4 * h)) = o;
                }
        }
        __syncthreads();                                          // d a2 of the wave's rows is in LDS
        // d x1^T (rows 64 q + c1, the wave's 32 rows (s2 = wave, pos)) = W2^T d a2^T, one child q at a time, and straight on through GELU
        // and LayerNorm 1 in the accumulators' layout: d1[half][i] belongs to sub-position s1 = 4 wave + q of position r, channel
        // 32 half + de_row(i, h).  Pass 1: d1 <- d z1 and the two row means; pass 2: d a1 and the channel sums, child after child.
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            f32x16 d1[2];
            const bf16x8* wp = static_cast<const bf16x8*>(A.pack_w2t) + (size_t)(2 * q) * (DG_DE_C2 / 16) * 64 + lane;
            const uint8_t* db = x1l + (size_t)(32 * wave + r) * DE_X1_PITCH + 16 * h;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int i = 0; i < 16; ++i) d1[hf][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < DG_DE_C2 / 16; ++ks) {
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(db + 32 * ks);
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) d1[hf] = DE_MFMA(wp[(hf * (DG_DE_C2 / 16) + ks) * 64], b, d1[hf]);
            }
            const int row = 32 * (4 * wave + q) + r;
            const f32x4 dv = *reinterpret_cast<const f32x4*>(dl + 4 * row);
            const float d[4] = {dv[0], dv[1], dv[2], dv[3]};
            const float mu = st[2 * row], rs = st[2 * row + 1];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = 32 * hf + de_row(i, h);
                    const float n = (de_a1(pl, d, c) - mu) * rs, g = pl[DG_DE_SP_G1 + c];
                    const float dz = d1[hf][i] * de_gelu_grad(fmaf(g, n, pl[DG_DE_SP_BE1 + c]));
                    d1[hf][i] = dz;
                    s1 = fmaf(dz, g, s1); s2 = fmaf(dz * g, n, s2);
                }
            s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            const float m1 = s1 * (1.f / DG_DE_C1), m2 = s2 * (1.f / DG_DE_C1);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = 32 * hf + de_row(i, h);
                    const float n = (de_a1(pl, d, c) - mu) * rs, dz = d1[hf][i];
                    const float da = rs * (dz * pl[DG_DE_SP_G1 + c] - m1 - n * m2);
                    float v[7] = {dz, dz * n, da, da * d[0], da * d[1], da * d[2], da * d[3]};
#pragma unroll
                    for (int k = 0; k < 7; ++k) v[k] = half_sum(v[k]);
                    if (r == 0) {                                 // (lanes 0 and 32: each owns its channels' slots of the wave's vector)
                        float* o[7] = {redw + DG_DE_SP_BE1 + c, redw + DG_DE_SP_G1 + c, redw + DG_DE_SP_B1 + c, redw + DG_DE_SP_W1 + 4 * c,
                                       redw + DG_DE_SP_W1 + 4 * c + 1, redw + DG_DE_SP_W1 + 4 * c + 2, redw + DG_DE_SP_W1 + 4 * c + 3};
#pragma unroll
                        for (int k = 0; k < 7; ++k) *o[k] = q == 0 ? v[k] : *o[k] + v[k];
                    }
                }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < DG_DE_SP; i += DE_THREADS)
            accl[i] += (red[i] + red[DG_DE_SP + i]) + (red[2 * DG_DE_SP + i] + red[3 * DG_DE_SP + i]);
        __syncthreads();                                          // the next tile writes the tiles and `red` again
    }
    for (int i = threadIdx.x; i < DG_DE_SP; i += DE_THREADS) A.part_small[(size_t)blockIdx.x * DG_DE_SP + i] = accl[i];
}

// ---- backward: d W2.  grid (4 children, splits_w2), block 256, static LDS.  One partial (in nn.Conv2d's order [c2][c1][q]) per split.
template <int C0>
__device__ __forceinline__ void de_x1_half(const float* pl, const float (&d)[4], float mu, float rstd, uint8_t* x1t, int row) {
#pragma unroll
    for (int c = C0; c < C0 + 32; ++c) *reinterpret_cast<__bf16*>(x1t + (size_t)c * DE_DA_PITCH + 2 * row) = (__bf16)de_x1(pl, d, mu, rstd, c);
}
__global__ __launch_bounds__(DE_THREADS) void k_de_bwd_w2(const DgDepthEncArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t x1t[DG_DE_C1 * DE_DA_PITCH];     // x1 of child q, [c1][row 32 s2 + pos] bf16
    __shared__ float pl[DG_DE_SP_B2];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31, h = lane >> 5;
    const int q = blockIdx.x, split = blockIdx.y;
    de_load_params(A, pl, false);
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int tile = split; tile < A.tiles; tile += A.splits_w2) {
        __syncthreads();                                          // the last tile's readers are done (the first: the parameters are in)
        {
            const int row = threadIdx.x & 127, s2 = row >> 5, pos = row & 31;
            float d[4], mu, rstd;
            de_load_depth(A, tile * DG_DE_TP + pos, 4 * s2 + q, d);
            de_s1_stats(pl, d, mu, rstd);
            if (threadIdx.x < 128) de_x1_half<0>(pl, d, mu, rstd, x1t, row);
            else de_x1_half<32>(pl, d, mu, rstd, x1t, row);
        }
        __syncthreads();
        const bf16x8* da = reinterpret_cast<const bf16x8*>(static_cast<const __bf16*>(A.da2t) + ((size_t)tile * DG_DE_C2 + 32 * wave + r) * 128 + 8 * h);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const bf16x8 a = da[2 * ks];
#pragma unroll
            for (int t = 0; t < 2; ++t)
                acc[t] = DE_MFMA(a, *reinterpret_cast<const bf16x8*>(x1t + (size_t)(32 * t + r) * DE_DA_PITCH + 32 * ks + 16 * h), acc[t]);
        }
    }
    float* part = A.part_w2 + (size_t)split * DG_DE_C2 * DG_DE_K2;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) part[(32 * wave + de_row(i, h)) * 256 + (32 * t + r) * 4 + q] = acc[t][i];
}

// ---- backward: d W3 and d b3.  grid (C / 64, splits_w3), block 256, no LDS.  One partial ([c][c2][s2], then d b3 as C high and C
// low floats) per split.
__global__ __launch_bounds__(DE_THREADS) void k_de_bwd_w3(const DgDepthEncArgs A) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31, h = lane >> 5;
    const int cb = blockIdx.x * 64, split = blockIdx.y;
    f32x16 acc[2][4];                                             // [channel tile][c2 tile of sub-position s2 = wave]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][t][i] = 0.f;
    double db = 0.0;                                              // d b3 of channel cb + (thread >> 2): 8 positions of every tile
    for (int tile = split; tile < A.tiles; tile += A.splits_w3) {
        const int n0 = tile * DG_DE_TP, b0 = n0 / A.P, p0 = n0 - b0 * A.P;
        bf16x8 a[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int j = 0; j < 8; ++j) a[m][ks][j] = (__bf16)de_g(A, n0, b0, p0, 16 * ks + 8 * h + j, cb + 32 * m + r);
        const __bf16* xb = static_cast<const __bf16*>(A.x2t) + ((size_t)tile * DG_DE_K3 + 128 * wave + r) * DG_DE_TP + 8 * h;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(xb + (size_t)32 * t * DG_DE_TP + 16 * ks);
#pragma unroll
                for (int m = 0; m < 2; ++m) acc[m][t] = DE_MFMA(a[m][ks], b, acc[m][t]);
            }
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += (double)de_g(A, n0, b0, p0, 8 * (threadIdx.x & 3) + j, cb + (threadIdx.x >> 2));
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        db += s;
    }
    float* part = A.part_w3 + (size_t)split * ((size_t)A.C * DG_DE_K3 + 2 * A.C);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) part[(size_t)(cb + 32 * m + de_row(i, h)) * DG_DE_K3 + (32 * t + r) * 4 + wave] = acc[m][t][i];
    if ((threadIdx.x & 3) == 0) {                                 // the fp64 sum as a float pair: no rounding to fp32 in front of the combine
        const float hi = (float)db;
        part[(size_t)A.C * DG_DE_K3 + cb + (threadIdx.x >> 2)] = hi;
        part[(size_t)A.C * DG_DE_K3 + A.C + cb + (threadIdx.x >> 2)] = (float)(db - (double)hi);
    }
}

// ---- the partials -> the gradients: out[i] = sum over k < count of part[k stride + i], fp64, four interleaved chains added pairwise.
// The n sums go to up to 8 tensors: segment s takes the indices end[s - 1] .. end[s] - 1.  grid ceil(n / 256), block 256.
// Indices from pair_from on are float pairs: the low halves stand pair_len further on.
struct DeCombine { const float* part; size_t stride; int count, n, nseg, pair_from, pair_len; float* dst[8]; int end[8]; };
__global__ __launch_bounds__(256) void k_de_combine(const DeCombine K) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K.n) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const float* src = K.part + i;
    int k = 0;
    for (; k + 4 <= K.count; k += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += (double)src[(size_t)(k + u) * K.stride];
    }
    for (int u = 0; k < K.count; ++k, ++u) s[u] += (double)src[(size_t)k * K.stride];
    if (i >= K.pair_from)
        for (k = 0; k < K.count; ++k) s[k & 3] += (double)src[(size_t)k * K.stride + K.pair_len];
    int seg = 0, first = 0;
    while (seg + 1 < K.nseg && i >= K.end[seg]) { first = K.end[seg]; ++seg; }
    K.dst[seg][i - first] = (float)((s[0] + s[1]) + (s[2] + s[3]));
}

static hipError_t de_pack(const DgDepthEncArgs& A, bool with_t, hipStream_t s) {
    const size_t items = ((size_t)DG_DE_C2 * DG_DE_K2 / 8 + (size_t)A.C * DG_DE_K3 / 8) * (with_t ? 2 : 1);
    hipLaunchKernelGGL(k_de_pack, dim3((unsigned)((items + DE_THREADS - 1) / DE_THREADS)), dim3(DE_THREADS), 0, s, A, with_t ? 1 : 0);
    return hipGetLastError();
}

hipError_t dg_launch_depthenc_forward(const DgDepthEncArgs& A, hipStream_t s) {
    hipError_t e = de_pack(A, false, s);
    if (e != hipSuccess) return e;
    return dg_launch(k_de_forward, dim3(A.tiles), dim3(DE_THREADS), de_fwd_lds(), s, A);
}

static hipError_t de_combine(const DeCombine& K, hipStream_t s) {
    hipLaunchKernelGGL(k_de_combine, dim3((K.n + 255) / 256), dim3(256), 0, s, K);
    return hipGetLastError();
}

hipError_t dg_launch_depthenc_backward(const DgDepthEncArgs& A, hipStream_t s) {
    hipError_t e = de_pack(A, true, s);
    if (e != hipSuccess) return e;
    const int lds = de_act_lds(A.C);
    if ((e = dg_launch(k_de_bwd_act, dim3(A.blocks_act), dim3(DE_THREADS), lds, s, A)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_de_bwd_w2, dim3(4, A.splits_w2), dim3(DE_THREADS), 0, s, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_de_bwd_w3, dim3(A.C / 64, A.splits_w3), dim3(DE_THREADS), 0, s, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    DeCombine K;
    memset(&K, 0, sizeof(K));
    K.part = A.part_small; K.stride = DG_DE_SP; K.count = A.blocks_act; K.n = K.pair_from = DG_DE_SP; K.nseg = 7;
    float* small[7] = {A.d_w1, A.d_b1, A.d_g1, A.d_be1, A.d_b2, A.d_g2, A.d_be2};
    const int ends[7] = {DG_DE_SP_B1, DG_DE_SP_G1, DG_DE_SP_BE1, DG_DE_SP_B2, DG_DE_SP_G2, DG_DE_SP_BE2, DG_DE_SP};
    for (int k = 0; k < 7; ++k) { K.dst[k] = small[k]; K.end[k] = ends[k]; }
    if ((e = de_combine(K, s)) != hipSuccess) return e;
    memset(&K, 0, sizeof(K));
    K.part = A.part_w2; K.stride = (size_t)DG_DE_C2 * DG_DE_K2; K.count = A.splits_w2; K.n = K.pair_from = DG_DE_C2 * DG_DE_K2; K.nseg = 1;
    K.dst[0] = A.d_w2; K.end[0] = K.n;
    if ((e = de_combine(K, s)) != hipSuccess) return e;
    memset(&K, 0, sizeof(K));
    K.part = A.part_w3; K.stride = (size_t)A.C * DG_DE_K3 + 2 * A.C; K.count = A.splits_w3; K.n = A.C * DG_DE_K3 + A.C; K.nseg = 2;
    K.pair_from = A.C * DG_DE_K3; K.pair_len = A.C;
    K.dst[0] = A.d_w3; K.end[0] = A.C * DG_DE_K3; K.dst[1] = A.d_b3; K.end[1] = K.n;
    return de_combine(K, s);
}
