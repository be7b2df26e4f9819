// Fused linear layers of the frozen DINO ViT (src/dino/vision_transformer.py:49-65, 68-92, 95-115):
//     y = epilogue(prologue(x) W^T + b)      x (M, K) row-major, W (Nout, K) as nn.Linear stores it
// prologue: LayerNorm over the row (norm1 -> qkv, norm2 -> fc1) or nothing; epilogue: exact GELU (fc1), residual add (proj, fc2), or
// nothing (qkv).  bf16 MFMA operands, fp32 accumulation, fp32 bias / GELU / residual.  DESIGN.md section 4.10 has the plan in prose.
//
//   k_lin_pack   rounds W to bf16 ONCE and stores it in the order the main kernel's MFMA fragments want it: per (tile of 32 output
//                columns, k-step of 16) one 1-KiB image [lane][8]: lane (r = lane & 31, h = lane >> 5) holds W[32 tile + r][16 ks + 8 h + j].
//                A wave that walks the k-steps of a column tile reads one contiguous stream, 16 bytes per lane.
//   k_lin_fwd    a workgroup = 4 waves owns a stripe of BM token rows.  It normalises (two passes over registers: mean, then the
//                centred squares) and rounds the stripe to bf16 ONCE into LDS, rows padded by 16 bytes (bank-conflict-free
//                ds_read_b128 of the fragments).  Then every wave walks its share of W's column blocks: the transposed product
//                    Y^T (cols x tokens) = W (A operand, straight from global / L2 in fragment order) x X^T (B operand, from LDS)
//                on mfma_f32_32x32x16_bf16, so a token sits on a lane and four consecutive output columns in four registers: the
//                epilogue reads the residual and writes the result with 128-bit accesses (64-bit for bf16 output).
//                No barrier after the staging one: W needs no LDS.  x is read from HBM once, LayerNorm computed once.
//                BM = 128 for K <= 384, 64 for K <= 768, 32 for K <= 1536, 16 for K <= 3072: the stripe is at most 98.5 KiB.
#include "dg_device.h"
#include "dg_aux_args.h"


#define LIN_WAVES 4
#define LIN_THREADS (64 * LIN_WAVES)
#define LIN_U 4                      // k-steps per prefetch group (K is a multiple of 64 = 4 k-steps)
#define LIN_LN_MAXV 12               // float4 per lane of a LayerNorm row held by 16 lanes: K <= 768

struct LinArgs {
    const void* x;                   // fp32 or bf16 (M, K)
    const float* gamma;              // LayerNorm weight / bias (K) or null
    const float* beta;
    const uint8_t* w;                // packed weight
    const float* bias;               // (Nout) or null
    const float* residual;           // (M, Nout) or null; may alias out
    void* out;                       // fp32 or bf16 (M, Nout)
    int M, K, Nout, bm;
    float eps;
    int flags;
};

__global__ __launch_bounds__(256) void k_lin_pack(const float* __restrict__ w, uint8_t* __restrict__ packed, int K, int Nout) {
    const int KS = K / 16;
    const size_t total = (size_t)(Nout / 32) * KS * 64;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= total) return;
    const int lane = (int)(c & 63), r = lane & 31, h = lane >> 5;
    const size_t f = c >> 6;
    const int ks = (int)(f % KS), tile = (int)(f / KS);
    const float* p = w + (size_t)(32 * tile + r) * K + 16 * ks + 8 * h;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    bf16x8 o;
    #pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] = (__bf16)a[j]; o[4 + j] = (__bf16)b[j]; }
    *reinterpret_cast<bf16x8*>(packed + c * 16) = o;
}

__device__ __forceinline__ float lin_sum16(float v) {           // sum over the 16 lanes that share a row
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
}

__device__ __forceinline__ bf16x4 lin_round4(f32x4 v) {
    bf16x4 o;
    #pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (__bf16)v[j];
    return o;
}

template <int MT, int NT>
__global__ __launch_bounds__(LIN_THREADS) void k_lin_fwd(LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lin_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int M = a.M, K = a.K, Nout = a.Nout, BM = a.bm;
    const int pitch = 2 * K + 16;                                   // bytes per LDS row
    const int row0 = blockIdx.x * BM;

    // ---- stage the stripe: prologue(x) rounded to bf16
    if (a.flags & DG_LIN_LAYERNORM) {
        const float* x = static_cast<const float*>(a.x);
        const int sub = lane & 15, kv = K / 64;                     // 16 lanes per row, kv float4 per lane
        for (int rl = wave * 4 + (lane >> 4); rl < BM; rl += 4 * LIN_WAVES) {
            const bool live = row0 + rl < M;
            const float* xr = x + (size_t)(live ? row0 + rl : M - 1) * K + 4 * sub;
            f32x4 v[LIN_LN_MAXV];
            #pragma unroll
            for (int i = 0; i < LIN_LN_MAXV; ++i)
                if (i < kv) v[i] = *reinterpret_cast<const f32x4*>(xr + 64 * i);
            float s = 0.f;
            #pragma unroll
            for (int i = 0; i < LIN_LN_MAXV; ++i)
                if (i < kv) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
            const float mean = lin_sum16(s) / (float)K;
            float q = 0.f;
            #pragma unroll
            for (int i = 0; i < LIN_LN_MAXV; ++i)
                if (i < kv) {
                    #pragma unroll
                    for (int j = 0; j < 4; ++j) { v[i][j] -= mean; q += v[i][j] * v[i][j]; }
                }
            const float rstd = 1.f / sqrtf(lin_sum16(q) / (float)K + a.eps);
            uint8_t* dst = lin_lds + (size_t)rl * pitch + 8 * sub;
            #pragma unroll
            for (int i = 0; i < LIN_LN_MAXV; ++i)
                if (i < kv) {
                    const f32x4 g = *reinterpret_cast<const f32x4*>(a.gamma + 4 * sub + 64 * i);
                    const f32x4 b = *reinterpret_cast<const f32x4*>(a.beta + 4 * sub + 64 * i);
                    f32x4 y;
                    #pragma unroll
                    for (int j = 0; j < 4; ++j) y[j] = live ? v[i][j] * rstd * g[j] + b[j] : 0.f;
                    *reinterpret_cast<bf16x4*>(dst + 128 * i) = lin_round4(y);
                }
        }
    } else if (a.flags & DG_LIN_IN_BF16) {
        const uint8_t* x = static_cast<const uint8_t*>(a.x);
        const int per = K / 8, total = BM * per;                    // 16-byte pieces
        for (int i0 = tid; i0 < total; i0 += 4 * LIN_THREADS) {
            u32x4 v[4];
            #pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int i = i0 + t * LIN_THREADS, rl = i / per, c = i - rl * per;
                v[t] = u32x4{0u, 0u, 0u, 0u};
                if (i < total && row0 + rl < M) v[t] = *reinterpret_cast<const u32x4*>(x + ((size_t)(row0 + rl) * K + 8 * c) * 2);
            }
            #pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int i = i0 + t * LIN_THREADS, rl = i / per, c = i - rl * per;
                if (i < total) *reinterpret_cast<u32x4*>(lin_lds + (size_t)rl * pitch + 16 * c) = v[t];
            }
        }
    } else {
        const float* x = static_cast<const float*>(a.x);
        const int per = K / 4, total = BM * per;                    // float4 pieces
        for (int i0 = tid; i0 < total; i0 += 8 * LIN_THREADS) {
            f32x4 v[8];
            #pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int i = i0 + t * LIN_THREADS, rl = i / per, c = i - rl * per;
                v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (i < total && row0 + rl < M) v[t] = *reinterpret_cast<const f32x4*>(x + (size_t)(row0 + rl) * K + 4 * c);
            }
            #pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int i = i0 + t * LIN_THREADS, rl = i / per, c = i - rl * per;
                if (i < total) *reinterpret_cast<bf16x4*>(lin_lds + (size_t)rl * pitch + 8 * c) = lin_round4(v[t]);
            }
        }
    }
    __syncthreads();

    // ---- the products: this wave's column blocks of 32 NT columns
    const int KS = K / 16, nblk = Nout / (32 * NT);
    const int rmask = BM < 32 ? BM - 1 : 31;                        // BM = 16: fragment rows 16..31 repeat rows 0..15 and are not written
    const bool out_bf16 = a.flags & DG_LIN_OUT_BF16, gelu = a.flags & DG_LIN_GELU;
    const bf16x8* wp = reinterpret_cast<const bf16x8*>(a.w);
    const uint8_t* xl = lin_lds + (size_t)(r & rmask) * pitch + 16 * h;      // + 32 mt rows, + 32 bytes per k-step

    for (int nb = wave; nb < nblk; nb += LIN_WAVES) {
        f32x16 acc[MT][NT];
        #pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            #pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                #pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;
        const bf16x8* wb = wp + (size_t)nb * NT * KS * 64 + lane;    // column tile nt: + nt KS 64; k-step: + 64
        bf16x8 wf[LIN_U][NT], wn[LIN_U][NT];
        #pragma unroll
        for (int u = 0; u < LIN_U; ++u)
            #pragma unroll
            for (int nt = 0; nt < NT; ++nt) wf[u][nt] = wb[((size_t)nt * KS + u) * 64];
        for (int ks0 = 0; ks0 < KS; ks0 += LIN_U) {
            const int kn = ks0 + LIN_U < KS ? ks0 + LIN_U : ks0;    // the last group re-reads itself: no branch around the loads
            #pragma unroll
            for (int u = 0; u < LIN_U; ++u)
                #pragma unroll
                for (int nt = 0; nt < NT; ++nt) wn[u][nt] = wb[((size_t)nt * KS + kn + u) * 64];
            #pragma unroll
            for (int u = 0; u < LIN_U; ++u) {
                bf16x8 xf[MT];
                #pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    xf[mt] = *reinterpret_cast<const bf16x8*>(xl + (size_t)(32 * mt) * pitch + 32 * (ks0 + u));
                #pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    #pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[u][nt], xf[mt], acc[mt][nt], 0, 0, 0);
            }
            #pragma unroll
            for (int u = 0; u < LIN_U; ++u)
                #pragma unroll
                for (int nt = 0; nt < NT; ++nt) wf[u][nt] = wn[u][nt];
        }

        // acc[mt][nt][i] = y[token 32 mt + r][column 32 (nb NT + nt) + (i & 3) + 8 (i >> 2) + 4 h] before bias
        #pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = 32 * (nb * NT + nt) + 8 * g + 4 * h;
                f32x4 b4 = f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.bias) b4 = *reinterpret_cast<const f32x4*>(a.bias + col);
                #pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int tl = 32 * mt + r;
                    if (tl >= BM || row0 + tl >= M) continue;
                    const size_t o = (size_t)(row0 + tl) * Nout + col;
                    f32x4 v;
                    #pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[j] = acc[mt][nt][4 * g + j] + b4[j];
                        if (gelu) v[j] = 0.5f * v[j] * (1.f + erff(v[j] * 0.70710678118654752440f));
                    }
                    if (a.residual) {
                        const f32x4 res = *reinterpret_cast<const f32x4*>(a.residual + o);
                        #pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = res[j] + v[j];
                    }
                    if (out_bf16) *reinterpret_cast<bf16x4*>(static_cast<__bf16*>(a.out) + o) = lin_round4(v);
                    else *reinterpret_cast<f32x4*>(static_cast<float*>(a.out) + o) = v;
                }
            }
    }
}

bool dg_linear_supported(int K, int Nout) {
    return K >= 64 && Nout >= 64 && K <= 3072 && Nout <= 3072 && K % 64 == 0 && Nout % 64 == 0;
}

size_t dg_linear_packed_bytes(int K, int Nout) { return dg_linear_supported(K, Nout) ? (size_t)K * Nout * 2 : 0; }

hipError_t dg_launch_linear_pack(const float* w, int K, int Nout, void* packed, hipStream_t s) {
    const size_t total = (size_t)(Nout / 32) * (K / 16) * 64;
    hipLaunchKernelGGL(k_lin_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, static_cast<uint8_t*>(packed), K, Nout);
    return hipGetLastError();
}

template <int MT, int NT>
static hipError_t lin_launch(const LinArgs& a, hipStream_t s) {
    const int lds = a.bm * (2 * a.K + 16);
    return dg_launch(k_lin_fwd<MT, NT>, dim3((a.M + a.bm - 1) / a.bm), dim3(LIN_THREADS), lds, s, a);
}

hipError_t dg_launch_linear(const void* x, const float* gamma, const float* beta, float eps, const void* packed, const float* bias,
                            const float* residual, void* out, int M, int K, int Nout, int flags, hipStream_t s) {
    LinArgs a{x, gamma, beta, static_cast<const uint8_t*>(packed), bias, residual, out, M, K, Nout, 0, eps, flags};
    a.bm = K <= 384 ? 128 : K <= 768 ? 64 : K <= 1536 ? 32 : 16;
    const bool wide = (Nout / 64) % LIN_WAVES == 0;                 // blocks of 64 columns share out evenly over the waves; else blocks of 32
    switch (a.bm) {
        case 128: return wide ? lin_launch<4, 2>(a, s) : lin_launch<4, 1>(a, s);
        case 64: return wide ? lin_launch<2, 2>(a, s) : lin_launch<2, 1>(a, s);
        default: return wide ? lin_launch<1, 2>(a, s) : lin_launch<1, 1>(a, s);
    }
}
