// Dense-CRF refinement of the evaluation (src/crf.py dense_crf, batched_crf of src/eval_segmentation.py:55-60, used at :162-167):
// mean-field inference of a fully connected CRF with two Potts terms (Kraehenbuehl & Koltun 2011), each message filtered on a
// permutohedral lattice (Adams et al. 2010), as densecrf 2.x (under pydensecrf) computes it:
//   Gaussian   features (x, y) / POS_XY_STD,                         weight POS_W, NORMALIZE_SYMMETRIC
//   bilateral  features (x, y) / Bi_XY_STD, (B, G, R) / Bi_RGB_STD,   weight Bi_W,  NORMALIZE_SYMMETRIC
//   Q0 = softmax(-U);  n_iter x  Q = softmax(-U + POS_W K~g(Q) + Bi_W K~b(Q)),  K~(Q) = norm . K(norm . Q),  norm = 1/sqrt(K(1) + 1e-20)
// Channels come in groups (one softmax each): the filter is linear and does not depend on the values, so the linear and the cluster
// probe of the evaluation (n + m channels) share one lattice build and one filter pass per iteration.
//
// Lattice build, per chunk of images (the image index sits above the key bits, so one sort serves the chunk):
//   k_crf_elevate    per pixel: the features, the elevated point, its simplex's d + 1 vertex keys (packed, dg_crf_key_plan) and
//                    barycentric weights; entry e = pixel * (d + 1) + r
//   sort             stable radix sort of (key, e) (dg_crf_sort.hip): the contributors of a vertex become one run, in entry order
//   k_crf_mark/scan  a flag per new key, its inclusive sum = 1 + the vertex number: vertices are numbered by their rank in key order
//   k_crf_vertices   the vertex of every entry, the run starts, the sorted unique keys and the vertex count (on the device: no sync)
//   k_crf_neighbours the two blur neighbours of every vertex in every direction by binary search in the sorted keys; a missing one
//                    points at the zero row (index Mcap, written by the call)
// Filter (values = fp32 rows of Kp channels, float4 loads and stores):
//   splat            gather over the sorted runs.  A run is cut at every multiple of CRF_TILE sorted positions of its image: the pieces after
//                    the first are summed per tile (k_crf_splat_tail), the first piece and then those partial sums in tile order by
//                    the vertex (k_crf_splat_head) - a fixed order, no atomics, and no thread walks more than CRF_TILE contributors
//                    plus one partial per tile of a long run (a flat colour region puts thousands of pixels on one vertex)
//   blur             one pass per direction j = 0..d: v' = v + 0.5 (v[n1] + v[n2]), ping-pong between two row buffers
//   slice            fused with the norms (folded into the splat and slice weights), alpha = 1 / (1 + 2^-d), the Potts weights,
//                    -U and the per-group softmax: one kernel per iteration (k_crf_step), which writes the next Q
// Every sum runs in an order fixed by the image's data alone, so two identical calls give identical bits, whatever the chunking.
#include "dg_device.h"
#include "dg_eval_args.h"
#include "dg_taps.h"          // resize_taps

#include <cmath>

// hipcc contracts a * b + c into an FMA by default, and HIP's __fmul_rn / __fadd_rn are plain operators defined in a header, out of
// reach of a pragma here: without these the colour chain and the elevation round differently from densecrf's (a colour one level
// off, a pixel in another simplex).  The sums that are meant to be fused say so with fmaf.
#pragma clang fp contract(off)
__device__ __forceinline__ float crf_mul(const float a, const float b) { return a * b; }
__device__ __forceinline__ float crf_add(const float a, const float b) { return a + b; }
__device__ __forceinline__ float crf_sub(const float a, const float b) { return a - b; }

#define CRF_THREADS 256
#define CRF_TILE 64           // splat: sorted contributors per partial sum
#define CRF_CLIP_LO 1e-5f     // pydensecrf.utils.unary_from_softmax: -log(clip(p, 1e-5, 1))

// UnNormalize (src/utils.py:132-136) then to_pil_image's mul(255).byte(): two fp32 roundings, then one more, then truncation.
// Values outside [0, 255] (undefined in the reference's byte()) are clamped.
__device__ __forceinline__ int crf_colour(const float v, const int c) {
    const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
    const float stdv = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    float t = crf_mul(crf_add(crf_mul(v, stdv), mean), 255.f);
    t = fminf(fmaxf(t, 0.f), 255.f);                                  // (NaN -> 0)
    return (int)t;
}

// ------------------------------------------------------------------------------------------------------------------- lattice build

struct CrfLat {               // one lattice of one chunk, in the workspace
    float* w;                 // [E] barycentric weight of entry e (pixel-major)
    int32_t* off;             // [E] vertex of entry e
    float* wl;                // [E] slice weight w * alpha * norm[pixel]
    int32_t* spix;            // [E] pixel of sorted position i
    float* sw;                // [E] splat weight of sorted position i: w (norm pass), then w * norm[pixel]
    int32_t* svid;            // [E] 1 + vertex of sorted position i
    int32_t* seg;             // [Mcap + 1] run start of vertex v (seg[M] = E)
    uint64_t* ukeys;          // [Mcap] sorted unique keys
    int32_t* nbr;             // [d + 1][Mcap][2] blur neighbours
    int32_t* M;               // vertex count
    float* norm;              // [N]
    float* V0; float* V1;     // [Mcap + 1][Kp] vertex rows (row Mcap: zeros)
    float* part;              // [tiles][Kp] partial splat sums
};
struct CrfSort { uint64_t* kin; uint64_t* kout; uint32_t* ein; uint32_t* eout; int32_t* flag; void* temp; size_t temp_bytes; };

template <int D>
__global__ __launch_bounds__(CRF_THREADS) void k_crf_elevate(const float* __restrict__ img, const int H, const int W, const int N,
                                                            const DgCrfKeys k, uint64_t* __restrict__ kin, uint32_t* __restrict__ ein,
                                                            float* __restrict__ wout) {
    const int p = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (p >= N) return;
    const int HW = H * W, im = p / HW, pix = p - im * HW, y = pix / W, x = pix - y * W;
    float f[D];
    f[0] = __fdiv_rn((float)x, k.stdv[0]);
    f[1] = __fdiv_rn((float)y, k.stdv[1]);
    if (D == 5) {
        const float* ip = img + (size_t)im * 3 * HW + pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) f[4 - c] = __fdiv_rn((float)crf_colour(ip[(size_t)c * HW], c), k.stdv[4 - c]);   // BGR
    }
    // elevate (densecrf's Permutohedral::init, fp32 without contraction)
    float el[D + 1];
    float sm = 0.f;
#pragma unroll
    for (int j = D; j > 0; --j) {
        const float cf = crf_mul(f[j - 1], k.scale[j - 1]);
        el[j] = crf_sub(sm, crf_mul((float)j, cf));
        sm = crf_add(sm, cf);
    }
    el[0] = sm;
    // the nearest remainder-0 point
    const float down = 1.f / (D + 1), up = (float)(D + 1);
    int rem0[D + 1], rank[D + 1];
    int sum = 0;
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        const float v = crf_mul(down, el[i]);
        const float hi = crf_mul(ceilf(v), up), lo = crf_mul(floorf(v), up);
        rem0[i] = crf_sub(hi, el[i]) < crf_sub(el[i], lo) ? (int)hi : (int)lo;
        sum += rem0[i] / (D + 1);
        rank[i] = 0;
    }
    float dl[D + 1];
#pragma unroll
    for (int i = 0; i <= D; ++i) dl[i] = crf_sub(el[i], (float)rem0[i]);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i + 1; j <= D; ++j) {
            if (dl[i] < dl[j]) ++rank[i];
            else ++rank[j];
        }
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        rank[i] += sum;
        if (rank[i] < 0) { rank[i] += D + 1; rem0[i] += D + 1; }
        else if (rank[i] > D) { rank[i] -= D + 1; rem0[i] -= D + 1; }
    }
    // barycentric weights: slot s gets +v of the coordinate of rank D - s and -v of the one of rank D - s + 1
    float vr[D + 1];
#pragma unroll
    for (int r = 0; r <= D; ++r) vr[r] = 0.f;
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        const float v = crf_mul(crf_sub(el[i], (float)rem0[i]), down);
#pragma unroll
        for (int r = 0; r <= D; ++r) vr[r] = rank[i] == r ? v : vr[r];
    }
    float bary[D + 1];
    bary[0] = (float)((double)vr[D] + (1.0 - (double)vr[0]));        // the wrap-around (densecrf: in double)
#pragma unroll
    for (int s = 1; s <= D; ++s) bary[s] = crf_sub(vr[D - s], vr[D - s + 1]);
    // the d + 1 vertices: rem0 + the canonical simplex's vertex r, first d coordinates
    const uint64_t base = (uint64_t)im << k.kbits;
#pragma unroll
    for (int r = 0; r <= D; ++r) {
        uint64_t key = base;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int c = rem0[i] + (rank[i] <= D - r ? r : r - (D + 1));
            key |= (uint64_t)(uint32_t)(c - k.lo[i]) << k.shift[i];
        }
        const size_t e = (size_t)p * (D + 1) + r;
        kin[e] = key;
        ein[e] = (uint32_t)e;
        wout[e] = bary[r];
    }
}

__global__ __launch_bounds__(CRF_THREADS) void k_crf_mark(const uint64_t* __restrict__ kout, int32_t* __restrict__ flag, const int E) {
    const int i = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (i >= E) return;
    flag[i] = (i == 0 || kout[i] != kout[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(CRF_THREADS) void k_crf_vertices(const CrfLat L, const CrfSort S, const int E, const int d1) {
    const int i = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (i >= E) return;
    const int v = L.svid[i] - 1;
    const uint32_t e = S.eout[i];
    L.off[e] = v;
    L.spix[i] = (int)(e / d1);
    L.sw[i] = L.w[e];
    if (S.flag[i]) { L.seg[v] = i; L.ukeys[v] = S.kout[i]; }
    if (i == E - 1) { *L.M = v + 1; L.seg[v + 1] = E; }
}

template <int D>
__global__ __launch_bounds__(CRF_THREADS) void k_crf_neighbours(const CrfLat L, const DgCrfKeys k, const int Mcap) {
    const int M = *L.M;
    for (int v = blockIdx.x * CRF_THREADS + threadIdx.x; v < M; v += gridDim.x * CRF_THREADS) {
        const uint64_t key = L.ukeys[v];
#pragma unroll
        for (int j = 0; j <= D; ++j) {
            uint64_t delta = 0;                                       // -1 on every coordinate, +d on coordinate j (n1); n2 = -n1
#pragma unroll
            for (int i = 0; i < D; ++i) delta += (uint64_t)(int64_t)(i == j ? D : -1) << k.shift[i];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const uint64_t want = t == 0 ? key + delta : key - delta;
                int lo = 0, hi = M;                                   // first index with ukeys >= want
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (L.ukeys[mid] < want) lo = mid + 1;
                    else hi = mid;
                }
                L.nbr[((size_t)j * Mcap + v) * 2 + t] = (lo < M && L.ukeys[lo] == want) ? lo : Mcap;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- filter

// a row of 4 channels of pixel p's values; ONES: the constant field (1, 0, 0, 0) of the norm pass
template <bool ONES>
__device__ __forceinline__ f32x4 crf_value(const float* __restrict__ X, const int p, const int Kp, const int q) {
    if (ONES) { f32x4 o = {1.f, 0.f, 0.f, 0.f}; return o; }
    return *reinterpret_cast<const f32x4*>(X + (size_t)p * Kp + 4 * q);
}

// Tiles are cut per image (image im owns the sorted positions [im E1, (im + 1) E1): its index sits above the key bits), so the cut
// points, and with them every sum, do not depend on which images share the chunk.
// partial sums of the tiles that continue a run begun in an earlier tile (written only for those; read only for those)
template <bool ONES>
__global__ __launch_bounds__(CRF_THREADS) void k_crf_splat_tail(const CrfLat L, const float* __restrict__ X, const int E, const int E1,
                                                               const int Kp) {
    const int Kq = Kp / 4, tpi = (E1 + CRF_TILE - 1) / CRF_TILE, tiles = (E / E1) * tpi;
    for (int idx = blockIdx.x * CRF_THREADS + threadIdx.x; idx < tiles * Kq; idx += gridDim.x * CRF_THREADS) {
        const int T = idx / Kq, q = idx - T * Kq, im = T / tpi, t = T - im * tpi, i0 = im * E1 + t * CRF_TILE;
        if (t == 0) continue;
        const int v = L.svid[i0];
        if (L.svid[i0 - 1] != v) continue;
        const int i1 = min((im + 1) * E1, i0 + CRF_TILE);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int i = i0; i < i1 && L.svid[i] == v; ++i) {
            const float w = L.sw[i];
            const f32x4 x = crf_value<ONES>(X, L.spix[i], Kp, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fmaf(w, x[c], acc[c]);
        }
        *reinterpret_cast<f32x4*>(L.part + (size_t)T * Kp + 4 * q) = acc;
    }
}

// vertex rows: the run's first piece, then the partial sums of the tiles it continues into, in tile order
template <bool ONES>
__global__ __launch_bounds__(CRF_THREADS) void k_crf_splat_head(const CrfLat L, const float* __restrict__ X, const int E1, const int Kp,
                                                               float* __restrict__ V) {
    const int Kq = Kp / 4, M = *L.M, tpi = (E1 + CRF_TILE - 1) / CRF_TILE;
    for (int idx = blockIdx.x * CRF_THREADS + threadIdx.x; idx < M * Kq; idx += gridDim.x * CRF_THREADS) {
        const int v = idx / Kq, q = idx - v * Kq;
        const int s = L.seg[v], e = L.seg[v + 1], im = s / E1, b0 = im * E1;
        const int t0 = (s - b0) / CRF_TILE, i1 = min(e, b0 + (t0 + 1) * CRF_TILE);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int i = s; i < i1; ++i) {
            const float w = L.sw[i];
            const f32x4 x = crf_value<ONES>(X, L.spix[i], Kp, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fmaf(w, x[c], acc[c]);
        }
        for (int t = t0 + 1; b0 + t * CRF_TILE < e; ++t) {
            const f32x4 pp = *reinterpret_cast<const f32x4*>(L.part + ((size_t)im * tpi + t) * Kp + 4 * q);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] += pp[c];
        }
        *reinterpret_cast<f32x4*>(V + (size_t)v * Kp + 4 * q) = acc;
    }
}

__global__ __launch_bounds__(CRF_THREADS) void k_crf_zero_rows(float* __restrict__ V0, float* __restrict__ V1, const int Mcap, const int Kp) {
    for (int c = threadIdx.x; c < Kp; c += CRF_THREADS) { V0[(size_t)Mcap * Kp + c] = 0.f; V1[(size_t)Mcap * Kp + c] = 0.f; }
}

__global__ __launch_bounds__(CRF_THREADS) void k_crf_blur(const CrfLat L, const int j, const int Mcap, const int Kp,
                                                         const float* __restrict__ vin, float* __restrict__ vout) {
    const int Kq = Kp / 4, M = *L.M;
    for (int idx = blockIdx.x * CRF_THREADS + threadIdx.x; idx < M * Kq; idx += gridDim.x * CRF_THREADS) {
        const int v = idx / Kq, q = idx - v * Kq;
        const int n1 = L.nbr[((size_t)j * Mcap + v) * 2], n2 = L.nbr[((size_t)j * Mcap + v) * 2 + 1];
        const f32x4 a = *reinterpret_cast<const f32x4*>(vin + (size_t)v * Kp + 4 * q);
        const f32x4 b = *reinterpret_cast<const f32x4*>(vin + (size_t)n1 * Kp + 4 * q);
        const f32x4 c = *reinterpret_cast<const f32x4*>(vin + (size_t)n2 * Kp + 4 * q);
        f32x4 o;
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = crf_add(a[t], crf_mul(0.5f, crf_add(b[t], c[t])));
        *reinterpret_cast<f32x4*>(vout + (size_t)v * Kp + 4 * q) = o;
    }
}

// K(1) (channel 0 of the ones pass) -> norm = 1 / sqrt(K(1) + 1e-20) (densecrf: in double)
__global__ __launch_bounds__(CRF_THREADS) void k_crf_norm(const CrfLat L, const float* __restrict__ V, const int N, const int d1,
                                                         const float alpha) {
    const int p = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (p >= N) return;
    float s = 0.f;
    for (int r = 0; r < d1; ++r) {
        const size_t e = (size_t)p * d1 + r;
        s = crf_add(s, crf_mul(crf_mul(L.w[e], V[(size_t)L.off[e] * 4]), alpha));
    }
    L.norm[p] = (float)(1.0 / sqrt((double)s + 1e-20));
}

// the norms folded into the weights: splat w * norm, slice w * alpha * norm
__global__ __launch_bounds__(CRF_THREADS) void k_crf_fold(const CrfLat L, const uint32_t* __restrict__ eout, const int E, const int d1,
                                                         const float alpha) {
    const int i = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (i >= E) return;
    L.sw[i] = crf_mul(L.w[eout[i]], L.norm[L.spix[i]]);
    L.wl[i] = crf_mul(crf_mul(L.w[i], alpha), L.norm[i / d1]);
}

// the message of one lattice at pixel p, 4 channels
__device__ __forceinline__ f32x4 crf_slice(const CrfLat& L, const float* __restrict__ V, const int p, const int d1, const int Kp,
                                           const int col) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < d1; ++r) {
        const size_t e = (size_t)p * d1 + r;
        const float w = L.wl[e];
        const f32x4 v = *reinterpret_cast<const f32x4*>(V + (size_t)L.off[e] * Kp + col);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = fmaf(w, v[c], acc[c]);
    }
    return acc;
}

// planar (B, C, H, W) values of the chunk -> pixel rows of Kp channels (padding 0)
__global__ __launch_bounds__(CRF_THREADS) void k_crf_pack(const float* __restrict__ in, float* __restrict__ X, const int N, const int HW,
                                                         const int C, const int Kp) {
    const int p = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (p >= N) return;
    const int im = p / HW, pix = p - im * HW;
    for (int c = 0; c < Kp; ++c) X[(size_t)p * Kp + c] = c < C ? in[((size_t)im * C + c) * HW + pix] : 0.f;
}

// dg_crf_filter's slice: the message, planar
__global__ __launch_bounds__(CRF_THREADS) void k_crf_slice_out(const CrfLat L, const float* __restrict__ V, float* __restrict__ out,
                                                              const int N, const int HW, const int C, const int Kp, const int d1) {
    const int p = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (p >= N) return;
    const int im = p / HW, pix = p - im * HW;
    for (int col = 0; col < Kp; col += 4) {
        const f32x4 m = crf_slice(L, V, p, d1, Kp, col);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (col + c < C) out[((size_t)im * C + col + c) * HW + pix] = m[c];
    }
}

// One mean-field update at pixel p: E = -U (+ w_pos K~g(Q) + w_bi K~b(Q) when LAT), Q = softmax(E) per group (the per-pixel maximum
// subtracted first).  Not FINAL: Q into the pixel rows X (read by this iteration's splats, which are done).  FINAL: Q planar (out)
// and / or the arg-max of each group (first maximum wins).  E is parked in X between the two passes of a group.
template <bool LAT, bool FINAL>
__global__ __launch_bounds__(CRF_THREADS) void k_crf_step(const DgCrfArgs a, const CrfLat Lg, const CrfLat Lb, const float* __restrict__ Vg,
                                                         const float* __restrict__ Vb, float* __restrict__ X, const int b0, const int N) {
    const int p = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (p >= N) return;
    const int HW = a.H * a.W, Kp = a.Kp, C = a.C;
    const int im = p / HW, pix = p - im * HW, b = b0 + im;
    float* xr = X + (size_t)p * Kp;
    for (int g = 0; g < a.G; ++g) {
        const int c0 = g ? a.gend[g - 1] : 0, c1 = a.gend[g], col0 = a.goff[g];
        float mx = -INFINITY;
        for (int c4 = c0; c4 < c1; c4 += 4) {
            const int col = col0 + (c4 - c0);
            f32x4 e;
#pragma unroll
            for (int t = 0; t < 4; ++t) e[t] = c4 + t < c1 ? -a.in[((size_t)b * C + c4 + t) * HW + pix] : 0.f;
            if (LAT) {
                const f32x4 kg = crf_slice(Lg, Vg, p, 3, Kp, col), kb = crf_slice(Lb, Vb, p, 6, Kp, col);
#pragma unroll
                for (int t = 0; t < 4; ++t) e[t] = crf_add(crf_add(e[t], crf_mul(a.w_pos, kg[t])), crf_mul(a.w_bi, kb[t]));
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (c4 + t < c1) mx = fmaxf(mx, e[t]);
            *reinterpret_cast<f32x4*>(xr + col) = e;
        }
        float sum = 0.f;
        for (int c4 = c0; c4 < c1; c4 += 4) {
            const int col = col0 + (c4 - c0);
            f32x4 e = *reinterpret_cast<const f32x4*>(xr + col);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                e[t] = c4 + t < c1 ? __expf(e[t] - mx) : 0.f;
                sum += e[t];
            }
            *reinterpret_cast<f32x4*>(xr + col) = e;
        }
        float best = -INFINITY;
        int arg = 0;
        for (int c4 = c0; c4 < c1; c4 += 4) {
            const int col = col0 + (c4 - c0);
            f32x4 e = *reinterpret_cast<const f32x4*>(xr + col);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                e[t] = c4 + t < c1 ? __fdiv_rn(e[t], sum) : 0.f;
                if (FINAL && c4 + t < c1) {
                    if (e[t] > best) { best = e[t]; arg = c4 + t - c0; }
                    if (a.out) a.out[((size_t)b * C + c4 + t) * HW + pix] = e[t];
                }
            }
            if (!FINAL) *reinterpret_cast<f32x4*>(xr + col) = e;
        }
        if (FINAL && a.preds) a.preds[((size_t)g * a.B + b) * HW + pix] = arg;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ host

static size_t crf_align(size_t x) { return (x + 255) / 256 * 256; }

bool dg_crf_key_plan(int d, int H, int W, const float* stdv, DgCrfKeys& k) {
    k = DgCrfKeys{};
    if ((d != 2 && d != 5) || H < 1 || W < 1) return false;
    k.d = d;
    double cmax[5];
    for (int i = 0; i < d; ++i) {
        if (!(stdv[i] > 0.f) || !std::isfinite(stdv[i])) return false;
        k.stdv[i] = stdv[i];
        k.scale[i] = (float)(1.0 / std::sqrt((double)(i + 2) * (i + 1)) * (std::sqrt(2.0 / 3.0) * (d + 1)));
        const double fmax = (i == 0 ? W - 1 : (i == 1 ? H - 1 : 255)) / (double)stdv[i];
        cmax[i] = fmax * (double)k.scale[i] * (1.0 + 1e-5) + 1e-3;
    }
    // elevated[0] in [0, sum c], elevated[j] in [-j c_{j-1}, sum_{i >= j} c_i]; a vertex key lies within 3 (d + 1) of the point, a blur
    // neighbour d further: a margin of 4 (d + 1) on either side keeps every key and every neighbour query inside its field
    int bits[5], total = 0;
    for (int i = 0; i < d; ++i) {
        double lo = 0.0, hi = 0.0;
        for (int t = i; t < d; ++t) hi += cmax[t];
        if (i > 0) lo = -i * cmax[i - 1];
        const double ulps = 1e-5 * (hi - lo);                       // the fp32 elevation's rounding at large coordinates
        lo = std::floor(lo - ulps) - 4.0 * (d + 1);
        hi = std::ceil(hi + ulps) + 4.0 * (d + 1);
        if (!(hi - lo < 2147483647.0)) return false;
        const uint64_t span = (uint64_t)(hi - lo) + 1;
        int nb = 1;
        while (nb < 63 && (1ull << nb) < span) ++nb;
        k.lo[i] = (int32_t)lo;
        bits[i] = nb;
        total += nb;
    }
    if (total > 63) return false;                                  // at least one bit for the image of the chunk
    int sh = 0;
    for (int i = d - 1; i >= 0; --i) { k.shift[i] = sh; sh += bits[i]; }
    k.kbits = total;
    return true;
}

int dg_crf_max_chunk(const DgCrfKeys& k) {
    const int free_bits = 64 - k.kbits;                             // >= 1 (dg_crf_key_plan)
    return free_bits >= 30 ? (1 << 30) : (1 << free_bits);
}

struct CrfWs {
    float* X;
    CrfLat lat[2];            // [0]: Gaussian (d = 2), [1]: bilateral (d = 5)
    CrfSort sort;
};

// the workspace of a chunk of c images for the lattices in `lats` (DG_CRF_GAUSSIAN | DG_CRF_BILATERAL): carved from `base` (null:
// sizes only); returns the bytes
static size_t crf_carve(char* base, const int c, const int HW, const int Kp, const int lats, CrfWs* ws) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += crf_align(bytes); return p; };
    const size_t N = (size_t)c * HW;
    CrfWs w{};
    w.X = reinterpret_cast<float*>(take(N * Kp * 4));
    for (int l = 0; l < 2; ++l) {
        if (!(lats & (l ? DG_CRF_BILATERAL : DG_CRF_GAUSSIAN))) continue;
        const int d1 = l ? 6 : 3;
        const size_t E = N * d1, Mcap = E, tiles = (size_t)c * (((size_t)HW * d1 + CRF_TILE - 1) / CRF_TILE);
        CrfLat& L = w.lat[l];
        L.w = reinterpret_cast<float*>(take(E * 4));
        L.off = reinterpret_cast<int32_t*>(take(E * 4));
        L.wl = reinterpret_cast<float*>(take(E * 4));
        L.spix = reinterpret_cast<int32_t*>(take(E * 4));
        L.sw = reinterpret_cast<float*>(take(E * 4));
        L.svid = reinterpret_cast<int32_t*>(take(E * 4));
        L.seg = reinterpret_cast<int32_t*>(take((Mcap + 1) * 4));
        L.ukeys = reinterpret_cast<uint64_t*>(take(Mcap * 8));
        L.nbr = reinterpret_cast<int32_t*>(take((size_t)d1 * Mcap * 2 * 4));
        L.M = reinterpret_cast<int32_t*>(take(4));
        L.norm = reinterpret_cast<float*>(take(N * 4));
        L.V0 = reinterpret_cast<float*>(take((Mcap + 1) * Kp * 4));
        L.V1 = reinterpret_cast<float*>(take((Mcap + 1) * Kp * 4));
        L.part = reinterpret_cast<float*>(take(tiles * Kp * 4));
    }
    const size_t E = N * ((lats & DG_CRF_BILATERAL) ? 6 : 3);
    w.sort.kin = reinterpret_cast<uint64_t*>(take(E * 8));
    w.sort.kout = reinterpret_cast<uint64_t*>(take(E * 8));
    w.sort.ein = reinterpret_cast<uint32_t*>(take(E * 4));
    w.sort.eout = reinterpret_cast<uint32_t*>(take(E * 4));
    w.sort.flag = reinterpret_cast<int32_t*>(take(E * 4));
    w.sort.temp_bytes = dg_crf_sort_temp_bytes((int)E);
    w.sort.temp = take(w.sort.temp_bytes);
    if (ws) *ws = w;
    return o;
}

// The kernels index entries and (vertex, 4-channel) pairs with int: a chunk is refused when (d + 1) c H W * Kp / 4 reaches 2^30.
size_t dg_crf_chunk_bytes(int c, int H, int W, int Kp, int lats) {
    if (c < 1 || H < 1 || W < 1 || Kp < 4 || Kp % 4 || (lats & ~3) || !lats || (long long)H * W > DG_CRF_MAX_HW) return 0;
    const long long d1 = (lats & DG_CRF_BILATERAL) ? 6 : 3;
    if ((long long)c * H * W * d1 * (Kp / 4) >= (1LL << 30)) return 0;
    return crf_carve(nullptr, c, H * W, Kp, lats, nullptr);
}

// the largest chunk of images the workspace holds (0: not even one)
static int crf_chunk(const DgCrfArgs& a, const int limit, const int lats) {
    int c = a.B < limit ? a.B : limit;
    while (c > 0) {
        const size_t need = dg_crf_chunk_bytes(c, a.H, a.W, a.Kp, lats);
        if (need && need <= a.ws_bytes) break;
        --c;
    }
    return c;
}

static dim3 crf_grid(const size_t work) {
    const size_t cap = (size_t)dg_cu_count() * 8;
    const size_t b = (work + CRF_THREADS - 1) / CRF_THREADS;
    return dim3((unsigned)(b < cap ? (b ? b : 1) : cap));
}
static dim3 crf_blocks(const size_t work) { return dim3((unsigned)((work + CRF_THREADS - 1) / CRF_THREADS)); }

#define CRF_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

// build lattice l of the chunk (N pixels from image pointer img) and its norms; on return L.sw / L.wl hold the folded weights
static hipError_t crf_build(const CrfWs& w, const int l, const DgCrfKeys& k, const float* img, const int H, const int W, const int N,
                            hipStream_t s) {
    const CrfLat& L = w.lat[l];
    const CrfSort& S = w.sort;
    const int d1 = k.d + 1, E = N * d1, Mcap = E;
    const float alpha = 1.f / (1.f + powf(2.f, -(float)k.d));
    if (k.d == 5) hipLaunchKernelGGL(k_crf_elevate<5>, crf_blocks(N), dim3(CRF_THREADS), 0, s, img, H, W, N, k, S.kin, S.ein, L.w);
    else hipLaunchKernelGGL(k_crf_elevate<2>, crf_blocks(N), dim3(CRF_THREADS), 0, s, img, H, W, N, k, S.kin, S.ein, L.w);
    CRF_TRY(hipGetLastError());
    int bits = k.kbits, cimg = (N / (H * W)) - 1;
    while (cimg > 0) { ++bits; cimg >>= 1; }
    CRF_TRY(dg_crf_sort_pairs(S.temp, S.temp_bytes, S.kin, S.kout, S.ein, S.eout, E, bits, s));
    hipLaunchKernelGGL(k_crf_mark, crf_blocks(E), dim3(CRF_THREADS), 0, s, S.kout, S.flag, E);
    CRF_TRY(hipGetLastError());
    CRF_TRY(dg_crf_scan(S.temp, S.temp_bytes, S.flag, L.svid, E, s));
    hipLaunchKernelGGL(k_crf_vertices, crf_blocks(E), dim3(CRF_THREADS), 0, s, L, S, E, d1);
    if (k.d == 5) hipLaunchKernelGGL(k_crf_neighbours<5>, crf_grid(Mcap), dim3(CRF_THREADS), 0, s, L, k, Mcap);
    else hipLaunchKernelGGL(k_crf_neighbours<2>, crf_grid(Mcap), dim3(CRF_THREADS), 0, s, L, k, Mcap);
    // K(1): the ones field through splat and blur (rows of 4), then the norms and the folded weights
    const int E1 = H * W * d1, tiles = (E / E1) * ((E1 + CRF_TILE - 1) / CRF_TILE);
    hipLaunchKernelGGL(k_crf_zero_rows, dim3(1), dim3(CRF_THREADS), 0, s, L.V0, L.V1, Mcap, 4);
    hipLaunchKernelGGL(k_crf_splat_tail<true>, crf_grid((size_t)tiles), dim3(CRF_THREADS), 0, s, L, (const float*)nullptr, E, E1, 4);
    hipLaunchKernelGGL(k_crf_splat_head<true>, crf_grid((size_t)Mcap), dim3(CRF_THREADS), 0, s, L, (const float*)nullptr, E1, 4, L.V0);
    float* src = L.V0; float* dst = L.V1;
    for (int j = 0; j < d1; ++j) {
        hipLaunchKernelGGL(k_crf_blur, crf_grid((size_t)Mcap), dim3(CRF_THREADS), 0, s, L, j, Mcap, 4, (const float*)src, dst);
        float* t = src; src = dst; dst = t;
    }
    hipLaunchKernelGGL(k_crf_norm, crf_blocks(N), dim3(CRF_THREADS), 0, s, L, (const float*)src, N, d1, alpha);
    hipLaunchKernelGGL(k_crf_fold, crf_blocks(E), dim3(CRF_THREADS), 0, s, L, (const uint32_t*)S.eout, E, d1, alpha);
    return hipGetLastError();
}

// the unnormalised filter K of the rows X (Kp channels) on lattice l, with the folded weights; returns the buffer holding the result
static const float* crf_filter_rows(const CrfWs& w, const int l, const int N, const int HW, const int Kp, hipStream_t s) {
    const CrfLat& L = w.lat[l];
    const int d1 = l ? 6 : 3, E = N * d1, Mcap = E, Kq = Kp / 4, E1 = HW * d1;
    const int tiles = (E / E1) * ((E1 + CRF_TILE - 1) / CRF_TILE);
    hipLaunchKernelGGL(k_crf_zero_rows, dim3(1), dim3(CRF_THREADS), 0, s, L.V0, L.V1, Mcap, Kp);
    hipLaunchKernelGGL(k_crf_splat_tail<false>, crf_grid((size_t)tiles * Kq), dim3(CRF_THREADS), 0, s, L, (const float*)w.X, E, E1, Kp);
    hipLaunchKernelGGL(k_crf_splat_head<false>, crf_grid((size_t)Mcap * Kq), dim3(CRF_THREADS), 0, s, L, (const float*)w.X, E1, Kp, L.V0);
    float* src = L.V0; float* dst = L.V1;
    for (int j = 0; j < d1; ++j) {
        hipLaunchKernelGGL(k_crf_blur, crf_grid((size_t)Mcap * Kq), dim3(CRF_THREADS), 0, s, L, j, Mcap, Kp, (const float*)src, dst);
        float* t = src; src = dst; dst = t;
    }
    return src;
}

hipError_t dg_launch_crf_filter(const DgCrfArgs& a, hipStream_t s) {
    const int l = a.filter_bilateral ? 1 : 0;
    const DgCrfKeys& k = l ? a.kb : a.kg;
    const int lats = l ? DG_CRF_BILATERAL : DG_CRF_GAUSSIAN;
    const int c = crf_chunk(a, dg_crf_max_chunk(k), lats);
    if (c < 1) return hipErrorInvalidValue;
    const int HW = a.H * a.W;
    CrfWs w;
    crf_carve(static_cast<char*>(a.ws), c, HW, a.Kp, lats, &w);
    for (int b0 = 0; b0 < a.B; b0 += c) {
        const int cc = a.B - b0 < c ? a.B - b0 : c, N = cc * HW;
        CRF_TRY(crf_build(w, l, k, a.img ? a.img + (size_t)b0 * 3 * HW : nullptr, a.H, a.W, N, s));
        hipLaunchKernelGGL(k_crf_pack, crf_blocks(N), dim3(CRF_THREADS), 0, s, a.in + (size_t)b0 * a.C * HW, w.X, N, HW, a.C, a.Kp);
        const float* V = crf_filter_rows(w, l, N, HW, a.Kp, s);
        hipLaunchKernelGGL(k_crf_slice_out, crf_blocks(N), dim3(CRF_THREADS), 0, s, w.lat[l], V, a.out + (size_t)b0 * a.C * HW, N, HW,
                           a.C, a.Kp, k.d + 1);
        CRF_TRY(hipGetLastError());
    }
    return hipSuccess;
}

hipError_t dg_launch_dense_crf(const DgCrfArgs& a, hipStream_t s) {
    const int lim_g = dg_crf_max_chunk(a.kg), lim_b = dg_crf_max_chunk(a.kb);
    const int lats = DG_CRF_GAUSSIAN | DG_CRF_BILATERAL;
    const int c = crf_chunk(a, lim_g < lim_b ? lim_g : lim_b, lats);
    if (c < 1) return hipErrorInvalidValue;
    const int HW = a.H * a.W;
    CrfWs w;
    crf_carve(static_cast<char*>(a.ws), c, HW, a.Kp, lats, &w);
    for (int b0 = 0; b0 < a.B; b0 += c) {
        const int cc = a.B - b0 < c ? a.B - b0 : c, N = cc * HW;
        const float* img = a.img + (size_t)b0 * 3 * HW;
        CRF_TRY(crf_build(w, 0, a.kg, img, a.H, a.W, N, s));
        CRF_TRY(crf_build(w, 1, a.kb, img, a.H, a.W, N, s));
        const dim3 grid = crf_blocks(N);
        if (a.n_iter == 0)
            hipLaunchKernelGGL((k_crf_step<false, true>), grid, dim3(CRF_THREADS), 0, s, a, w.lat[0], w.lat[1], (const float*)nullptr,
                               (const float*)nullptr, w.X, b0, N);
        else
            hipLaunchKernelGGL((k_crf_step<false, false>), grid, dim3(CRF_THREADS), 0, s, a, w.lat[0], w.lat[1], (const float*)nullptr,
                               (const float*)nullptr, w.X, b0, N);
        for (int it = 0; it < a.n_iter; ++it) {
            const float* Vg = crf_filter_rows(w, 0, N, HW, a.Kp, s);
            const float* Vb = crf_filter_rows(w, 1, N, HW, a.Kp, s);
            if (it == a.n_iter - 1)
                hipLaunchKernelGGL((k_crf_step<true, true>), grid, dim3(CRF_THREADS), 0, s, a, w.lat[0], w.lat[1], Vg, Vb, w.X, b0, N);
            else
                hipLaunchKernelGGL((k_crf_step<true, false>), grid, dim3(CRF_THREADS), 0, s, a, w.lat[0], w.lat[1], Vg, Vb, w.X, b0, N);
        }
        CRF_TRY(hipGetLastError());
    }
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------------------------------ unary

// U = -log(clip(softmax(z), 1e-5, 1)) over channels [c0, c1) of one pixel; z(c) gives the logit of channel c
template <class Z>
__device__ __forceinline__ void crf_write_unary(const Z& z, const int c0, const int c1, float* __restrict__ U, const size_t stride) {
    float mx = -INFINITY;
    for (int c = c0; c < c1; ++c) mx = fmaxf(mx, z(c));
    float sum = 0.f;
    for (int c = c0; c < c1; ++c) sum += __expf(z(c) - mx);
    for (int c = c0; c < c1; ++c) {
        const float pr = fminf(fmaxf(__fdiv_rn(__expf(z(c) - mx), sum), CRF_CLIP_LO), 1.f);
        U[c * stride] = -__logf(pr);
    }
}

// bilinear blend of F.interpolate (align_corners=False): h0 (w0 a + w1 b) + h1 (w0 c + w1 d)
__device__ __forceinline__ float crf_blend(const float a, const float b, const float c, const float d, const float lx, const float ly) {
    const float top = crf_add(crf_mul(1.f - lx, a), crf_mul(lx, b));
    const float bot = crf_add(crf_mul(1.f - lx, c), crf_mul(lx, d));
    return crf_add(crf_mul(1.f - ly, top), crf_mul(ly, bot));
}

// generic: logits (B, C, h, w) at any resolution -> U (B, C, H, W), one softmax per group
struct CrfUnaryArgs { const float* logits; float* U; int32_t B, C, h, w, H, W, G; int32_t gend[DG_CRF_MAX_GROUPS]; };
__global__ __launch_bounds__(CRF_THREADS) void k_crf_unary(const CrfUnaryArgs a) {
    const int HW = a.H * a.W;
    const long long gp = (long long)blockIdx.x * CRF_THREADS + threadIdx.x;
    if (gp >= (long long)a.B * HW) return;
    const int b = (int)(gp / HW), pix = (int)(gp - (long long)b * HW), Y = pix / a.W, X = pix - Y * a.W;
    int y0, y1, x0, x1; float ly, lx;
    resize_taps(Y, a.h, a.H, y0, y1, ly);
    resize_taps(X, a.w, a.W, x0, x1, lx);
    const size_t hw = (size_t)a.h * a.w;
    const float* base = a.logits + (size_t)b * a.C * hw;
    const int q00 = y0 * a.w + x0, q01 = y0 * a.w + x1, q10 = y1 * a.w + x0, q11 = y1 * a.w + x1;
    const auto z = [=](int c) {
        const float* q = base + c * hw;
        return crf_blend(q[q00], q[q01], q[q10], q[q11], lx, ly);
    };
    for (int g = 0; g < a.G; ++g)
        crf_write_unary(z, g ? a.gend[g - 1] : 0, a.gend[g], a.U + (size_t)b * a.C * HW + pix, HW);
}

// eval route: the projected score rows (k_seg_project: (B, h*w, n4 + m4)) resized per label pixel; the cluster rows divided by the
// resized code's norm and scaled by alpha (ClusterLookup(..., alpha=2, log_probs=True) on F.interpolate(code)) -> U (B, n + m, H, W)
__global__ __launch_bounds__(CRF_THREADS) void k_seg_unary(const DgSegArgs a, const float alpha, float* __restrict__ U) {
    const int HW = a.H * a.W;
    const long long gp = (long long)blockIdx.x * CRF_THREADS + threadIdx.x;
    if (gp >= (long long)a.B * HW) return;
    const int b = (int)(gp / HW), pix = (int)(gp - (long long)b * HW), Y = pix / a.W, X = pix - Y * a.W;
    int y0, y1, x0, x1; float ly, lx;
    resize_taps(Y, a.h, a.H, y0, y1, ly);
    resize_taps(X, a.w, a.W, x0, x1, lx);
    const int hw = a.h * a.w, Kp = dg_seg_kp(a.n, a.m), n4 = (a.n + 3) / 4 * 4, C = a.n + a.m;
    // |interp(code)| at this pixel (the flip form: of (code + code_flip.flip(3)) / 2)
    const int q00 = y0 * a.w + x0, q01 = y0 * a.w + x1, q10 = y1 * a.w + x0, q11 = y1 * a.w + x1;
    const float* cp = a.code + (size_t)b * a.D * hw;
    const float* fp = a.code_flip ? a.code_flip + (size_t)b * a.D * hw : nullptr;
    const int f00 = y0 * a.w + (a.w - 1 - x0), f01 = y0 * a.w + (a.w - 1 - x1), f10 = y1 * a.w + (a.w - 1 - x0), f11 = y1 * a.w + (a.w - 1 - x1);
    float ss = 0.f;
    for (int d = 0; d < a.D; ++d) {
        const float* c = cp + (size_t)d * hw;
        float v00 = c[q00], v01 = c[q01], v10 = c[q10], v11 = c[q11];
        if (fp) {
            const float* f = fp + (size_t)d * hw;
            v00 = (v00 + f[f00]) * 0.5f; v01 = (v01 + f[f01]) * 0.5f; v10 = (v10 + f[f10]) * 0.5f; v11 = (v11 + f[f11]) * 0.5f;
        }
        const float v = crf_blend(v00, v01, v10, v11, lx, ly);
        ss = fmaf(v, v, ss);
    }
    const float scl = alpha / fmaxf(sqrtf(ss), DG_EPS_NORM_DEFAULT);
    const float* s00 = a.scores + ((size_t)b * hw + q00) * Kp, *s01 = a.scores + ((size_t)b * hw + q01) * Kp;
    const float* s10 = a.scores + ((size_t)b * hw + q10) * Kp, *s11 = a.scores + ((size_t)b * hw + q11) * Kp;
    float* ub = U + (size_t)b * C * HW + pix;
    const int n = a.n;
    const auto zl = [=](int c) { return crf_blend(s00[c], s01[c], s10[c], s11[c], lx, ly); };
    const auto zc = [=](int c) { const int k = n4 + c - n; return crf_blend(s00[k], s01[k], s10[k], s11[k], lx, ly) * scl; };
    crf_write_unary(zl, 0, n, ub, HW);
    crf_write_unary(zc, n, C, ub, HW);
}

hipError_t dg_launch_crf_unary(const float* logits, int B, int C, int h, int w, int H, int W, int G, const int32_t* gend, float* U,
                               hipStream_t s) {
    CrfUnaryArgs a{logits, U, B, C, h, w, H, W, G, {}};
    for (int g = 0; g < G; ++g) a.gend[g] = gend[g];
    hipLaunchKernelGGL(k_crf_unary, crf_blocks((size_t)B * H * W), dim3(CRF_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t dg_launch_segment_unary(const DgSegArgs& a, float alpha, float* U, hipStream_t s) {
    CRF_TRY(dg_launch_seg_project(a, s));
    hipLaunchKernelGGL(k_seg_unary, crf_blocks((size_t)a.B * a.H * a.W), dim3(CRF_THREADS), 0, s, a, alpha, U);
    return hipGetLastError();
}
