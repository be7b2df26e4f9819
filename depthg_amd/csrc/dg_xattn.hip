// Fused cross-attention of the depth guidance (src/modules.py:524, :566-585: nn.MultiheadAttention(n_feats, 8, dropout=0.1) between
// depth queries and image tokens), forward AND backward, with the Nq x Nk matrix kept in registers.  Head dimension 48, separate
// query and key / value tensors, attention dropout from Philox.  DESIGN.md section 4.17 has the plan in prose.
//
//   k_xattn_pack  one (B, N, heads * 48) fp32 tensor -> bf16 MFMA fragments, stored ONCE per call: per (b, head, tile of 32 rows) one
//                 7-KiB image
//                     [0, 3 KiB)   row fragments   [ks = 0..2][lane][8]   : lane (r = lane & 31, h = lane >> 5) holds X[row r][d = 16 ks + 8 h + j]
//                     [3, 7 KiB)   X^T fragments   [db][s][lane][8]       : lane (r, h) holds X[row 16 s + 8 (j >> 2) + 4 h + (j & 3)][d = 32 db + r]
//                 (the row order of an X^T fragment is the accumulator-row order of a 32x32 MFMA tile: the operand that meets it comes
//                 straight out of the registers of the product before).  Rows >= N and d >= 48 are zeros: no kernel reads past an image.
//                 A row fragment serves as the A operand (rows on the output's rows) and as the B operand (rows on its columns) alike.
//   k_xattn_fwd   a wave = 32 queries of one (b, head), a workgroup = 4 waves.  Per tile of 32 keys, as k_attn_fwd (dg_attn.hip):
//                     S^T = K Q^T (3 k-steps) -> online softmax in fp32, query on the lane -> dropout -> O^T += V^T P^T (2 x 2, d padded to 64)
//   k_xattn_prep  Di = rowsum(dO * O) and the log-sum-exp in log2 units, both padded to whole tiles (+inf / 0 behind Nq: such a
//                 row's probabilities re-form as exact zeros)
//   k_xattn_dq    a wave = 32 queries; per key tile  S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (keep / (1 - p) dP^T - Di), dQ^T += K^T dS^T
//   k_xattn_dkv   a wave = 32 keys;    per query tile S = Q K^T,  dP = dO V^T,  dV^T += dO^T Pd,  dK^T += Q^T dS
//   k_xattn_mask  the keep decisions as bytes
// The fragments are read from the images with one 16-byte load per lane (1 KiB per wave, consecutive); no LDS, no barrier, no atomics:
// every output element has one owner that sums in one fixed order.
//
// Dropout: element (b, head, q, k) is kept iff word (k & 3) of Philox4x32-10(key = seed, counter = (q, k >> 2, head, b)) >= floor(p 2^32).
// The counter holds each index in a 32-bit word of its own: nothing of the shape, the tiles or the grid enters, and no shape can wrap it.
#include "dg_device.h"
#include "dg_aux_args.h"

#define XA_TILE 32                    // rows per image
#define XA_WAVES 4
#define XA_ROWS_WG (32 * XA_WAVES)    // queries (keys, in k_xattn_dkv) per workgroup
#define XA_FRAG_T 3                   // index of the first X^T fragment in an image

__device__ __forceinline__ bool xa_keep(uint32_t word, uint32_t thr) { return word >= thr; }

__device__ __forceinline__ const bf16x8* xa_image(const uint8_t* img, size_t tile) {
    return reinterpret_cast<const bf16x8*>(img + tile * DG_XATTN_IMG);
}

__global__ __launch_bounds__(256) void k_xattn_pack(const float* __restrict__ x, uint8_t* __restrict__ img, int N, int heads, int tiles) {
    const int tile = blockIdx.x, bh = blockIdx.y, b = bh / heads, head = bh % heads;
    const size_t row = (size_t)heads * DG_XATTN_HD;                // floats per token
    const float* base = x + (size_t)b * N * row + (size_t)head * DG_XATTN_HD;
    uint8_t* out = img + ((size_t)bh * tiles + tile) * DG_XATTN_IMG;
    for (int c = threadIdx.x; c < 7 * 64; c += 256) {
        const int lane = c & 63, r = lane & 31, h = lane >> 5, f = c >> 6;
        bf16x8 o;
        #pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (__bf16)0.f;
        if (f < XA_FRAG_T) {                                        // row fragment of k-step f
            const int key = tile * XA_TILE + r;
            if (key < N) {
                const float* p = base + (size_t)key * row + 16 * f + 8 * h;
                const f32x4 a = *reinterpret_cast<const f32x4*>(p), bq = *reinterpret_cast<const f32x4*>(p + 4);
                #pragma unroll
                for (int j = 0; j < 4; ++j) { o[j] = (__bf16)a[j]; o[4 + j] = (__bf16)bq[j]; }
            }
        } else {                                                    // X^T fragment of d-block (f - 3) >> 1, k-step (f - 3) & 1
            const int d = 32 * ((f - XA_FRAG_T) >> 1) + r, s = (f - XA_FRAG_T) & 1;
            if (d < DG_XATTN_HD) {
                #pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int key = tile * XA_TILE + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
                    if (key < N) o[j] = (__bf16)base[(size_t)key * row + d];
                }
            }
        }
        *reinterpret_cast<bf16x8*>(out + (size_t)c * 16) = o;
    }
}

// acc[db][i] = X^T[d = 32 db + (i & 3) + 8 (i >> 2) + 4 h][row on the lane] -> X[row][d], times `f`; d < 48 only
__device__ __forceinline__ void xa_store_rows(float* __restrict__ dst, const f32x16 (&acc)[2], float f, int h) {
    #pragma unroll
    for (int db = 0; db < 2; ++db)
        #pragma unroll
        for (int g = 0; g < (db ? 2 : 4); ++g) {
            f32x4 v;
            #pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[db][4 * g + j] * f;
            *reinterpret_cast<f32x4*>(dst + 32 * db + 8 * g + 4 * h) = v;
        }
}

template <bool DROP>
__global__ __launch_bounds__(64 * XA_WAVES) void k_xattn_fwd(const float* __restrict__ q, const uint8_t* __restrict__ img_k,
                                                            const uint8_t* __restrict__ img_v, float* __restrict__ out,
                                                            float* __restrict__ lse, int Nq, int Nk, int heads, int tiles_k,
                                                            float scale_log2e, uint64_t seed, uint32_t thr, float inv_keep) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / heads, head = bh % heads;
    const int q0 = blockIdx.x * XA_ROWS_WG + wave * 32;
    if (q0 >= Nq) return;                                           // wave-uniform; the kernel has no barrier
    const int qi = q0 + r, qc = qi < Nq ? qi : Nq - 1;              // tail queries read the last row and are not written
    const size_t row = (size_t)heads * DG_XATTN_HD;

    bf16x8 qf[3];                                                   // B operand of S^T = K Q^T: lane (r, h) holds Q[query r][d = 16 ks + 8 h + j]
    {
        const float* p = q + ((size_t)b * Nq + qc) * row + (size_t)head * DG_XATTN_HD + 8 * h;
        #pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(p + 16 * ks), bq = *reinterpret_cast<const f32x4*>(p + 16 * ks + 4);
            #pragma unroll
            for (int j = 0; j < 4; ++j) { qf[ks][j] = (__bf16)a[j]; qf[ks][4 + j] = (__bf16)bq[j]; }
        }
    }

    f32x16 acc[2];
    #pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
    float m = -INFINITY, l = 0.f;                                   // running maximum (log2 units) and this lane's half of the sum

    bf16x8 kf[3], vf[4], kn[3], vn[4];
    {
        const bf16x8* ik = xa_image(img_k, (size_t)bh * tiles_k), * iv = xa_image(img_v, (size_t)bh * tiles_k);
        #pragma unroll
        for (int f = 0; f < 3; ++f) kf[f] = ik[f * 64 + lane];
        #pragma unroll
        for (int f = 0; f < 4; ++f) vf[f] = iv[(XA_FRAG_T + f) * 64 + lane];
    }
    for (int t = 0; t < tiles_k; ++t) {
        if (t + 1 < tiles_k) {                                      // the next tile's fragments travel under this tile's products
            const bf16x8* ik = xa_image(img_k, (size_t)bh * tiles_k + t + 1), * iv = xa_image(img_v, (size_t)bh * tiles_k + t + 1);
            #pragma unroll
            for (int f = 0; f < 3; ++f) kn[f] = ik[f * 64 + lane];
            #pragma unroll
            for (int f = 0; f < 4; ++f) vn[f] = iv[(XA_FRAG_T + f) * 64 + lane];
        }
        f32x16 s;
        #pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
        #pragma unroll
        for (int ks = 0; ks < 3; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
        // s[i] = score of (query on the lane, key (i & 3) + 8 (i >> 2) + 4 h of the tile)
        #pragma unroll
        for (int i = 0; i < 16; ++i) s[i] *= scale_log2e;
        if ((t + 1) * XA_TILE > Nk) {                               // the last tile: tail keys leave the maximum and the sum
            const int k0 = t * XA_TILE + 4 * h;
            #pragma unroll
            for (int i = 0; i < 16; ++i)
                if (k0 + (i & 3) + 8 * (i >> 2) >= Nk) s[i] = -INFINITY;
        }
        float mx = s[0];
        #pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);                              // finite: every tile holds at least one key < Nk
        const float alpha = __builtin_amdgcn_exp2f(m - mn);         // 0 on the first tile (m = -inf)
        m = mn;
        float sum = 0.f, p[16];
        #pragma unroll
        for (int i = 0; i < 16; ++i) { p[i] = __builtin_amdgcn_exp2f(s[i] - mn); sum += p[i]; }
        if (DROP) {                                                 // the row sum is the softmax's: it keeps the dropped keys
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u32x4 w = dg_philox4(seed, (uint32_t)qi, (uint32_t)(t * 8 + 2 * g + h), (uint32_t)head, (uint32_t)b);
                #pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (!xa_keep(w[j], thr)) p[4 * g + j] = 0.f;
            }
        }
        bf16x8 pf[2];
        #pragma unroll
        for (int i = 0; i < 16; ++i) pf[i >> 3][i & 7] = (__bf16)p[i];
        l = l * alpha + sum;
        #pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] *= alpha; acc[1][i] *= alpha; }
        #pragma unroll
        for (int db = 0; db < 2; ++db)
            #pragma unroll
            for (int ss = 0; ss < 2; ++ss)
                acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[db * 2 + ss], pf[ss], acc[db], 0, 0, 0);
        #pragma unroll
        for (int f = 0; f < 3; ++f) kf[f] = kn[f];
        #pragma unroll
        for (int f = 0; f < 4; ++f) vf[f] = vn[f];
    }

    l += __shfl_xor(l, 32);
    if (qi < Nq) {
        xa_store_rows(out + ((size_t)b * Nq + qi) * row + (size_t)head * DG_XATTN_HD, acc, inv_keep / l, h);
        if (lse && h == 0) lse[(size_t)bh * Nq + qi] = (m + __builtin_amdgcn_logf(l)) * 0.69314718055994530942f;   // v_log_f32 is log2
    }
}

// lse2p, dip: (B * heads, tiles_q * 32) - the rows of a tile in one aligned run, whatever Nq is
__global__ __launch_bounds__(64) void k_xattn_prep(const float* __restrict__ o, const float* __restrict__ d_o, const float* __restrict__ lse,
                                                  float* __restrict__ lse2p, float* __restrict__ dip, int Nq, int heads, int tiles_q) {
    const int bh = blockIdx.y, b = bh / heads, head = bh % heads;
    const int qi = blockIdx.x * 64 + threadIdx.x;
    if (qi >= tiles_q * XA_TILE) return;
    float di = 0.f, l2 = INFINITY;
    if (qi < Nq) {
        const size_t off = ((size_t)b * Nq + qi) * ((size_t)heads * DG_XATTN_HD) + (size_t)head * DG_XATTN_HD;
        #pragma unroll
        for (int c = 0; c < DG_XATTN_HD; c += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(o + off + c), g = *reinterpret_cast<const f32x4*>(d_o + off + c);
            #pragma unroll
            for (int j = 0; j < 4; ++j) di += a[j] * (float)(__bf16)g[j];   // d O as the products see it: dP and Di then cancel where they must
        }
        l2 = lse[(size_t)bh * Nq + qi] * 1.44269504088896340736f;
    }
    lse2p[(size_t)bh * tiles_q * XA_TILE + qi] = l2;
    dip[(size_t)bh * tiles_q * XA_TILE + qi] = di;
}

template <bool DROP>
__global__ __launch_bounds__(64 * XA_WAVES) void k_xattn_dq(const uint8_t* __restrict__ img_q, const uint8_t* __restrict__ img_do,
                                                           const uint8_t* __restrict__ img_k, const uint8_t* __restrict__ img_v,
                                                           const float* __restrict__ lse2p, const float* __restrict__ dip,
                                                           float* __restrict__ dq, int Nq, int Nk, int heads, int tiles_q, int tiles_k,
                                                           float scale, float scale_log2e, uint64_t seed, uint32_t thr, float inv_keep) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / heads, head = bh % heads;
    const int tq = blockIdx.x * XA_WAVES + wave, q0 = tq * XA_TILE;
    if (q0 >= Nq) return;
    const int qi = q0 + r;

    bf16x8 qf[3], dof[3];                                           // B operands: lane (r, h) holds X[query r][d = 16 ks + 8 h + j]
    {
        const bf16x8* iq = xa_image(img_q, (size_t)bh * tiles_q + tq), * io = xa_image(img_do, (size_t)bh * tiles_q + tq);
        #pragma unroll
        for (int f = 0; f < 3; ++f) { qf[f] = iq[f * 64 + lane]; dof[f] = io[f * 64 + lane]; }
    }
    const float lse2 = lse2p[(size_t)bh * tiles_q * XA_TILE + qi], di = dip[(size_t)bh * tiles_q * XA_TILE + qi];

    f32x16 acc[2];
    #pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }

    bf16x8 kf[3], vf[3], kt[4], kn[3], vn[3], ktn[4];
    {
        const bf16x8* ik = xa_image(img_k, (size_t)bh * tiles_k), * iv = xa_image(img_v, (size_t)bh * tiles_k);
        #pragma unroll
        for (int f = 0; f < 3; ++f) { kf[f] = ik[f * 64 + lane]; vf[f] = iv[f * 64 + lane]; }
        #pragma unroll
        for (int f = 0; f < 4; ++f) kt[f] = ik[(XA_FRAG_T + f) * 64 + lane];
    }
    for (int t = 0; t < tiles_k; ++t) {
        if (t + 1 < tiles_k) {
            const bf16x8* ik = xa_image(img_k, (size_t)bh * tiles_k + t + 1), * iv = xa_image(img_v, (size_t)bh * tiles_k + t + 1);
            #pragma unroll
            for (int f = 0; f < 3; ++f) { kn[f] = ik[f * 64 + lane]; vn[f] = iv[f * 64 + lane]; }
            #pragma unroll
            for (int f = 0; f < 4; ++f) ktn[f] = ik[(XA_FRAG_T + f) * 64 + lane];
        }
        f32x16 s, dp;
        #pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
        #pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);        // S^T[key][query]
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[ks], dof[ks], dp, 0, 0, 0);     // dP^T[key][query] = V dO^T
        }
        float p[16];
        #pragma unroll
        for (int i = 0; i < 16; ++i) p[i] = __builtin_amdgcn_exp2f(s[i] * scale_log2e - lse2);      // lse2 = +inf behind Nq: 0
        if ((t + 1) * XA_TILE > Nk) {                               // tail keys (zero rows of K: a score of 0, not a probability of 0)
            const int k0 = t * XA_TILE + 4 * h;
            #pragma unroll
            for (int i = 0; i < 16; ++i)
                if (k0 + (i & 3) + 8 * (i >> 2) >= Nk) p[i] = 0.f;
        }
        if (DROP) {
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u32x4 w = dg_philox4(seed, (uint32_t)qi, (uint32_t)(t * 8 + 2 * g + h), (uint32_t)head, (uint32_t)b);
                #pragma unroll
                for (int j = 0; j < 4; ++j) dp[4 * g + j] = xa_keep(w[j], thr) ? dp[4 * g + j] * inv_keep : 0.f;
            }
        }
        bf16x8 dsf[2];
        #pragma unroll
        for (int i = 0; i < 16; ++i) dsf[i >> 3][i & 7] = (__bf16)(p[i] * (dp[i] - di));
        #pragma unroll
        for (int db = 0; db < 2; ++db)
            #pragma unroll
            for (int ss = 0; ss < 2; ++ss)
                acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt[db * 2 + ss], dsf[ss], acc[db], 0, 0, 0);   // dQ^T += K^T dS^T
        #pragma unroll
        for (int f = 0; f < 3; ++f) { kf[f] = kn[f]; vf[f] = vn[f]; }
        #pragma unroll
        for (int f = 0; f < 4; ++f) kt[f] = ktn[f];
    }
    if (qi < Nq)
        xa_store_rows(dq + ((size_t)b * Nq + qi) * ((size_t)heads * DG_XATTN_HD) + (size_t)head * DG_XATTN_HD, acc, scale, h);
}

template <bool DROP>
__global__ __launch_bounds__(64 * XA_WAVES) void k_xattn_dkv(const uint8_t* __restrict__ img_q, const uint8_t* __restrict__ img_do,
                                                            const uint8_t* __restrict__ img_k, const uint8_t* __restrict__ img_v,
                                                            const float* __restrict__ lse2p, const float* __restrict__ dip,
                                                            float* __restrict__ dk, float* __restrict__ dv, int Nq, int Nk, int heads,
                                                            int tiles_q, int tiles_k, float scale, float scale_log2e, uint64_t seed,
                                                            uint32_t thr, float inv_keep) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / heads, head = bh % heads;
    const int tk = blockIdx.x * XA_WAVES + wave, k0 = tk * XA_TILE;
    if (k0 >= Nk) return;
    const int ki = k0 + r;
    const bool key_live = ki < Nk;

    bf16x8 kf[3], vf[3];                                            // B operands: lane (r, h) holds X[key r][d = 16 ks + 8 h + j]
    {
        const bf16x8* ik = xa_image(img_k, (size_t)bh * tiles_k + tk), * iv = xa_image(img_v, (size_t)bh * tiles_k + tk);
        #pragma unroll
        for (int f = 0; f < 3; ++f) { kf[f] = ik[f * 64 + lane]; vf[f] = iv[f * 64 + lane]; }
    }
    f32x16 acc_k[2], acc_v[2];
    #pragma unroll
    for (int i = 0; i < 16; ++i) { acc_k[0][i] = 0.f; acc_k[1][i] = 0.f; acc_v[0][i] = 0.f; acc_v[1][i] = 0.f; }
    const float* lrow = lse2p + (size_t)bh * tiles_q * XA_TILE + 4 * h, * drow = dip + (size_t)bh * tiles_q * XA_TILE + 4 * h;

    for (int t = 0; t < tiles_q; ++t) {
        const bf16x8* iq = xa_image(img_q, (size_t)bh * tiles_q + t), * io = xa_image(img_do, (size_t)bh * tiles_q + t);
        bf16x8 qf[3], dof[3], qt[4], dot[4];
        #pragma unroll
        for (int f = 0; f < 3; ++f) { qf[f] = iq[f * 64 + lane]; dof[f] = io[f * 64 + lane]; }
        #pragma unroll
        for (int f = 0; f < 4; ++f) { qt[f] = iq[(XA_FRAG_T + f) * 64 + lane]; dot[f] = io[(XA_FRAG_T + f) * 64 + lane]; }
        f32x4 l4[4], d4[4];                                          // element j of group g: query 8 g + 4 h + j of the tile = accumulator row 4 g + j
        #pragma unroll
        for (int g = 0; g < 4; ++g) {
            l4[g] = *reinterpret_cast<const f32x4*>(lrow + t * XA_TILE + 8 * g);
            d4[g] = *reinterpret_cast<const f32x4*>(drow + t * XA_TILE + 8 * g);
        }
        f32x16 s, dp;
        #pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
        #pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], kf[ks], s, 0, 0, 0);        // S[query][key]
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof[ks], vf[ks], dp, 0, 0, 0);     // dP[query][key] = dO V^T
        }
        bf16x8 pdf[2], dsf[2];
        #pragma unroll
        for (int i = 0; i < 16; ++i) {
            float p = __builtin_amdgcn_exp2f(s[i] * scale_log2e - l4[i >> 2][i & 3]);       // +inf behind Nq: 0
            if (!key_live) p = 0.f;
            float pd = p, dpm = dp[i];
            if (DROP) {
                const int qi = t * XA_TILE + (i & 3) + 8 * (i >> 2) + 4 * h;
                const u32x4 w = dg_philox4(seed, (uint32_t)qi, (uint32_t)(ki >> 2), (uint32_t)head, (uint32_t)b);
                const uint32_t w01 = (ki & 1) ? w[1] : w[0], w23 = (ki & 1) ? w[3] : w[2];
                const bool keep = xa_keep((ki & 2) ? w23 : w01, thr);
                pd = keep ? p : 0.f;
                dpm = keep ? dpm * inv_keep : 0.f;
            }
            pdf[i >> 3][i & 7] = (__bf16)pd;
            dsf[i >> 3][i & 7] = (__bf16)(p * (dpm - d4[i >> 2][i & 3]));
        }
        #pragma unroll
        for (int db = 0; db < 2; ++db)
            #pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                acc_v[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot[db * 2 + ss], pdf[ss], acc_v[db], 0, 0, 0);   // dV^T += dO^T Pd
                acc_k[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt[db * 2 + ss], dsf[ss], acc_k[db], 0, 0, 0);    // dK^T += Q^T dS
            }
    }
    if (key_live) {
        const size_t off = ((size_t)b * Nk + ki) * ((size_t)heads * DG_XATTN_HD) + (size_t)head * DG_XATTN_HD;
        xa_store_rows(dk + off, acc_k, scale, h);
        xa_store_rows(dv + off, acc_v, inv_keep, h);
    }
}

// one thread per (b, head, q, four keys): the four words of one Philox call
__global__ __launch_bounds__(256) void k_xattn_mask(uint8_t* __restrict__ out, long long quads, int Nq, int Nk, int heads, uint64_t seed,
                                                   uint32_t thr, bool drop) {
    const int k4n = (Nk + 3) >> 2;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < quads; idx += (long long)gridDim.x * 256) {
        const int k4 = (int)(idx % k4n);
        const long long rowi = idx / k4n;                           // (b * heads + head) * Nq + q
        const int qi = (int)(rowi % Nq), bh = (int)(rowi / Nq);
        u32x4 w = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        if (drop) w = dg_philox4(seed, (uint32_t)qi, (uint32_t)k4, (uint32_t)(bh % heads), (uint32_t)(bh / heads));
        uint8_t* o = out + rowi * Nk + 4 * (long long)k4;
        #pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * k4 + j < Nk) o[j] = xa_keep(w[j], thr) ? 1 : 0;
    }
}

DgXattnWs dg_xattn_ws(int B, int heads, int Nq, int Nk, bool backward) {
    DgXattnWs w;
    w.tiles_q = (Nq + XA_TILE - 1) / XA_TILE;
    w.tiles_k = (Nk + XA_TILE - 1) / XA_TILE;
    const size_t bh = (size_t)B * heads, iq = bh * w.tiles_q * DG_XATTN_IMG, ik = bh * w.tiles_k * DG_XATTN_IMG;   // (multiples of 256)
    size_t at = 0;
    w.img_k = at; at += ik;
    w.img_v = at; at += ik;
    w.img_q = w.img_do = w.lse2 = w.di = 0;
    if (backward) {
        const size_t rows = (bh * w.tiles_q * XA_TILE * sizeof(float) + 255) / 256 * 256;
        w.img_q = at; at += iq;
        w.img_do = at; at += iq;
        w.lse2 = at; at += rows;
        w.di = at; at += rows;
    }
    w.total = at;
    return w;
}

static hipError_t xa_pack(const float* x, uint8_t* img, int BH, int N, int heads, int tiles, hipStream_t s) {
    hipLaunchKernelGGL(k_xattn_pack, dim3(tiles, BH), dim3(256), 0, s, x, img, N, heads, tiles);
    return hipGetLastError();
}

hipError_t dg_launch_xattn_forward(const DgXattnArgs& A, hipStream_t s) {
    const DgXattnWs w = dg_xattn_ws(A.B, A.heads, A.Nq, A.Nk, false);
    uint8_t* base = static_cast<uint8_t*>(A.workspace);
    const int BH = A.B * A.heads;
    hipError_t e = xa_pack(A.k, base + w.img_k, BH, A.Nk, A.heads, w.tiles_k, s);
    if (e != hipSuccess) return e;
    e = xa_pack(A.v, base + w.img_v, BH, A.Nk, A.heads, w.tiles_k, s);
    if (e != hipSuccess) return e;
    const dim3 grid((A.Nq + XA_ROWS_WG - 1) / XA_ROWS_WG, BH), block(64 * XA_WAVES);
    const float sl2 = A.scale * 1.44269504088896340736f;
    if (A.thr)
        hipLaunchKernelGGL(k_xattn_fwd<true>, grid, block, 0, s, A.q, base + w.img_k, base + w.img_v, A.out_w, A.lse_w, A.Nq, A.Nk, A.heads,
                           w.tiles_k, sl2, A.seed, A.thr, A.inv_keep);
    else
        hipLaunchKernelGGL(k_xattn_fwd<false>, grid, block, 0, s, A.q, base + w.img_k, base + w.img_v, A.out_w, A.lse_w, A.Nq, A.Nk, A.heads,
                           w.tiles_k, sl2, A.seed, 0u, 1.f);
    return hipGetLastError();
}

hipError_t dg_launch_xattn_backward(const DgXattnArgs& A, hipStream_t s) {
    const DgXattnWs w = dg_xattn_ws(A.B, A.heads, A.Nq, A.Nk, true);
    uint8_t* base = static_cast<uint8_t*>(A.workspace);
    const int BH = A.B * A.heads;
    hipError_t e = xa_pack(A.k, base + w.img_k, BH, A.Nk, A.heads, w.tiles_k, s);
    if (e != hipSuccess) return e;
    e = xa_pack(A.v, base + w.img_v, BH, A.Nk, A.heads, w.tiles_k, s);
    if (e != hipSuccess) return e;
    e = xa_pack(A.q, base + w.img_q, BH, A.Nq, A.heads, w.tiles_q, s);
    if (e != hipSuccess) return e;
    e = xa_pack(A.d_out, base + w.img_do, BH, A.Nq, A.heads, w.tiles_q, s);
    if (e != hipSuccess) return e;
    float* lse2p = reinterpret_cast<float*>(base + w.lse2), * dip = reinterpret_cast<float*>(base + w.di);
    hipLaunchKernelGGL(k_xattn_prep, dim3((w.tiles_q * XA_TILE + 63) / 64, BH), dim3(64), 0, s, A.out, A.d_out, A.lse, lse2p, dip, A.Nq,
                       A.heads, w.tiles_q);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const float sl2 = A.scale * 1.44269504088896340736f;
    const bool drop = A.thr != 0;
    const uint32_t thr = drop ? A.thr : 0u;
    const float inv_keep = drop ? A.inv_keep : 1.f;
    const dim3 block(64 * XA_WAVES);
    if (A.d_q) {
        const dim3 grid((A.Nq + XA_ROWS_WG - 1) / XA_ROWS_WG, BH);
        if (drop)
            hipLaunchKernelGGL(k_xattn_dq<true>, grid, block, 0, s, base + w.img_q, base + w.img_do, base + w.img_k, base + w.img_v, lse2p, dip,
                               A.d_q, A.Nq, A.Nk, A.heads, w.tiles_q, w.tiles_k, A.scale, sl2, A.seed, thr, inv_keep);
        else
            hipLaunchKernelGGL(k_xattn_dq<false>, grid, block, 0, s, base + w.img_q, base + w.img_do, base + w.img_k, base + w.img_v, lse2p, dip,
                               A.d_q, A.Nq, A.Nk, A.heads, w.tiles_q, w.tiles_k, A.scale, sl2, A.seed, thr, inv_keep);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (A.d_k) {
        const dim3 grid((A.Nk + XA_ROWS_WG - 1) / XA_ROWS_WG, BH);
        if (drop)
            hipLaunchKernelGGL(k_xattn_dkv<true>, grid, block, 0, s, base + w.img_q, base + w.img_do, base + w.img_k, base + w.img_v, lse2p, dip,
                               A.d_k, A.d_v, A.Nq, A.Nk, A.heads, w.tiles_q, w.tiles_k, A.scale, sl2, A.seed, thr, inv_keep);
        else
            hipLaunchKernelGGL(k_xattn_dkv<false>, grid, block, 0, s, base + w.img_q, base + w.img_do, base + w.img_k, base + w.img_v, lse2p, dip,
                               A.d_k, A.d_v, A.Nq, A.Nk, A.heads, w.tiles_q, w.tiles_k, A.scale, sl2, A.seed, thr, inv_keep);
        e = hipGetLastError();
    }
    return e;
}

hipError_t dg_launch_xattn_mask(uint8_t* out, int B, int heads, int Nq, int Nk, uint64_t seed, uint32_t thr, hipStream_t s) {
    const long long quads = (long long)B * heads * Nq * ((Nk + 3) / 4);
    const long long want = (quads + 255) / 256;
    const int blocks = (int)(want < (1ll << 20) ? want : (1ll << 20));
    hipLaunchKernelGGL(k_xattn_mask, dim3(blocks), dim3(256), 0, s, out, quads, Nq, Nk, heads, seed, thr, thr != 0);
    return hipGetLastError();
}
