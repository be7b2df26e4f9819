// Fused attention forward of the frozen DINO ViT (src/dino/vision_transformer.py:80-92): softmax(q k^T * scale) v per (batch, head)
// with the N x N matrix kept in registers (online softmax).  Head dimension 64.  DESIGN.md section 4.9 has the plan in prose.
//
//   k_attn_pack   reads K and V out of the packed fp32 (B, N, 3, heads, 64) tensor the qkv linear wrote and stores them ONCE as bf16
//                 in the order the main kernel's MFMA fragments want them: per (b, head, tile of 32 keys) one 8-KiB image
//                     [0, 4 KiB)   K fragments  [ks = 0..3][lane][8]   : lane (r = lane & 31, h = lane >> 5) holds K[key r][d = 16 ks + 8 h + j]
//                     [4, 8 KiB)   V^T fragments [db][s][lane][8]      : lane (r, h) holds V[key 16 s + 8 (j >> 2) + 4 h + (j & 3)][d = 32 db + r]
//                 (the k order of the V^T fragment is the accumulator-row order of a 32x32 MFMA tile, cdna guide section 3 "An accumulator
//                 tile as the next MFMA's operand").  Keys >= N are stored as zeros: the main kernel never reads past an image.
//   k_attn_fwd    a workgroup = 4 waves = 128 queries of one (b, head); a wave owns 32 queries.  Per tile of 32 keys:
//                     S^T = K Q^T          4 x mfma_f32_32x32x16_bf16  (A = K fragment from LDS, B = Q fragment, held in registers)
//                                          -> lane (q = lane & 31, h) holds the scores of query q against 16 of the 32 keys
//                     online softmax       fp32: the running maximum needs 15 max + 1 exchange with lane ^ 32, the factor exp(m_old - m_new)
//                                          is per LANE because the query sits on the lane in S^T and in O^T alike
//                     O^T += V^T P^T       4 x mfma (A = V^T fragment from LDS, B = P rounded to bf16 straight out of the registers)
//                 The 8-KiB image of the next tile is fetched into registers before the products of this one and stored to the other
//                 half of a 16-KiB LDS ring after them: one barrier per tile.
#include "dg_device.h"
#include "dg_aux_args.h"

#define ATT_HD 64
#define ATT_TILE 32                 // keys per tile
#define ATT_WAVES 4
#define ATT_QWG (32 * ATT_WAVES)    // queries per workgroup
#define ATT_IMG 8192                // bytes of one packed tile image


__global__ __launch_bounds__(256) void k_attn_pack(const float* __restrict__ qkv, uint8_t* __restrict__ kv, int N, int heads, int tiles) {
    const int tile = blockIdx.x, bh = blockIdx.y, b = bh / heads, head = bh % heads;
    const size_t row = (size_t)3 * heads * ATT_HD;                 // floats per token
    const float* base = qkv + (size_t)b * N * row + (size_t)head * ATT_HD;
    uint8_t* img = kv + ((size_t)bh * tiles + tile) * ATT_IMG;
    for (int c = threadIdx.x; c < 512; c += 256) {
        const int lane = c & 63, r = lane & 31, h = lane >> 5, f = (c >> 6) & 3;
        bf16x8 o;
        if (c < 256) {                                              // K fragment of k-step f
            const int key = tile * ATT_TILE + r;
            if (key < N) {
                const float* p = base + (size_t)key * row + (size_t)heads * ATT_HD + 16 * f + 8 * h;
                const f32x4 a = *reinterpret_cast<const f32x4*>(p), bq = *reinterpret_cast<const f32x4*>(p + 4);
                #pragma unroll
                for (int j = 0; j < 4; ++j) { o[j] = (__bf16)a[j]; o[4 + j] = (__bf16)bq[j]; }
            } else {
                #pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (__bf16)0.f;
            }
        } else {                                                    // V^T fragment of d-block f >> 1, k-step f & 1
            const int d = 32 * (f >> 1) + r, s = f & 1;
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = tile * ATT_TILE + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
                o[j] = key < N ? (__bf16)base[(size_t)key * row + (size_t)2 * heads * ATT_HD + d] : (__bf16)0.f;
            }
        }
        *reinterpret_cast<bf16x8*>(img + (size_t)c * 16) = o;
    }
}

__global__ __launch_bounds__(64 * ATT_WAVES, 2) void k_attn_fwd(const float* __restrict__ qkv, const uint8_t* __restrict__ kv,
                                                                 float* __restrict__ out, int N, int heads, int tiles, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[2][ATT_IMG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / heads, head = bh % heads;
    const int q0 = blockIdx.x * ATT_QWG + wave * 32;
    const bool live = q0 < N;                                       // wave-uniform: a wave past the last query only helps to stage
    const int q = q0 + r < N ? q0 + r : N - 1;                      // tail queries read the last row and are not written
    const size_t row = (size_t)3 * heads * ATT_HD;

    // Q fragments (B operand of S^T = K Q^T): lane (r, h) holds Q[query r][d = 16 ks + 8 h + j]
    bf16x8 qf[4];
    {
        const float* p = qkv + ((size_t)b * N + q) * row + (size_t)head * ATT_HD + 8 * h;
        #pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(p + 16 * ks), bq = *reinterpret_cast<const f32x4*>(p + 16 * ks + 4);
            #pragma unroll
            for (int j = 0; j < 4; ++j) { qf[ks][j] = (__bf16)a[j]; qf[ks][4 + j] = (__bf16)bq[j]; }
        }
    }

    const u32x4* src = reinterpret_cast<const u32x4*>(kv + (size_t)bh * tiles * ATT_IMG);     // 512 x 16 bytes per tile
    u32x4 st0 = src[tid], st1 = src[256 + tid];
    reinterpret_cast<u32x4*>(ring[0])[tid] = st0;
    reinterpret_cast<u32x4*>(ring[0])[256 + tid] = st1;
    __syncthreads();

    f32x16 acc[2];
    #pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
    float m = -INFINITY, l = 0.f;                                   // running maximum (in log2 units) and this lane's half of the sum

    for (int t = 0; t < tiles; ++t) {
        if (t + 1 < tiles) {
            st0 = src[(size_t)(t + 1) * 512 + tid];
            st1 = src[(size_t)(t + 1) * 512 + 256 + tid];
        }
        if (live) {
            const bf16x8* img = reinterpret_cast<const bf16x8*>(ring[t & 1]);
            f32x16 s;
            #pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f;
            #pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(img[ks * 64 + lane], qf[ks], s, 0, 0, 0);
            // s[i] = score of (query r, key (i & 3) + 8 (i >> 2) + 4 h of the tile)
            #pragma unroll
            for (int i = 0; i < 16; ++i) s[i] *= scale_log2e;
            if ((t + 1) * ATT_TILE > N) {                           // the last tile: tail keys leave the maximum and the sum
                const int k0 = t * ATT_TILE + 4 * h;
                #pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (k0 + (i & 3) + 8 * (i >> 2) >= N) s[i] = -INFINITY;
            }
            float mx = s[0];
            #pragma unroll
            for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m, mx);                          // finite: every tile holds at least one key < N
            const float alpha = __builtin_amdgcn_exp2f(m - mn);     // 0 on the first tile (m = -inf)
            m = mn;
            float sum = 0.f;
            bf16x8 pf[2];
            #pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = __builtin_amdgcn_exp2f(s[i] - mn);
                sum += p;
                pf[i >> 3][i & 7] = (__bf16)p;
            }
            l = l * alpha + sum;
            #pragma unroll
            for (int i = 0; i < 16; ++i) { acc[0][i] *= alpha; acc[1][i] *= alpha; }
            #pragma unroll
            for (int db = 0; db < 2; ++db)
                #pragma unroll
                for (int ss = 0; ss < 2; ++ss)
                    acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(img[256 + (db * 2 + ss) * 64 + lane], pf[ss], acc[db], 0, 0, 0);
        }
        if (t + 1 < tiles) {
            reinterpret_cast<u32x4*>(ring[(t + 1) & 1])[tid] = st0;
            reinterpret_cast<u32x4*>(ring[(t + 1) & 1])[256 + tid] = st1;
        }
        __syncthreads();
    }

    // acc[db][i] = O[query r][d = 32 db + (i & 3) + 8 (i >> 2) + 4 h] * l
    l += __shfl_xor(l, 32);
    if (live && q0 + r < N) {
        const float inv = 1.f / l;
        float* o = out + ((size_t)b * N + q0 + r) * ((size_t)heads * ATT_HD) + (size_t)head * ATT_HD + 4 * h;
        #pragma unroll
        for (int db = 0; db < 2; ++db)
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
                #pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[db][4 * g + j] * inv;
                *reinterpret_cast<f32x4*>(o + 32 * db + 8 * g) = v;
            }
    }
}

size_t dg_attn_workspace(int B, int heads, int N) {
    const size_t tiles = ((size_t)N + ATT_TILE - 1) / ATT_TILE;
    return (size_t)B * heads * tiles * ATT_IMG;
}

hipError_t dg_launch_attention(const float* qkv, float* out, void* ws, int B, int N, int heads, float scale, hipStream_t s) {
    const int tiles = (N + ATT_TILE - 1) / ATT_TILE;
    uint8_t* kv = static_cast<uint8_t*>(ws);
    hipLaunchKernelGGL(k_attn_pack, dim3(tiles, B * heads), dim3(256), 0, s, qkv, kv, N, heads, tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_attn_fwd, dim3((N + ATT_QWG - 1) / ATT_QWG, B * heads), dim3(64 * ATT_WAVES), 0, s, qkv, kv, out, N, heads, tiles,
                       scale * 1.44269504088896340736f);
    return hipGetLastError();
}
