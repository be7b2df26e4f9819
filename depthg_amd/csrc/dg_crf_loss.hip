// The contrastive CRF loss term of the training step (cfg.crf_weight): ContrastiveCRFLoss (src/modules.py:1510-1542) with its caller's
// resize, norm and mean (src/train_segmentation.py:413-419; src/utils.py:60-61, src/modules.py:789-790) as three kernels.  With S_a the
// normalised, resized code vector at sample a of one image and K_ac the (symmetric) similarity kernel of the sample coordinates and
// the resized image colours,
//     mean(-sims * K) = -(1 / (B n^2)) sum_b sum_a S_a . G_a,   G_a = sum_c K_ac S_c,   d mean / d S_a = -(2 / (B n^2)) G_a:
// one pass that forms G gives the loss and everything the backward needs.  Nothing of size (B,n,n) or size x size is written.
//   k_crfl_sample    the two bilinear resizes AT the n sampled positions only, the norm: S (B,n,Dp), |x| (B,n), g (B,n,4)
//   k_crfl_pair      G = K S per image with K formed on the fly, q_a = S_a . G_a / |S_a|^2, one fp64 partial sum per block
//   k_loss_reduce    the partial sums -> the loss scalar (fp64, fixed order; dg_loss_reduce.hip)
//   k_crfl_backward  d code, destination-major: one block per (image, code pixel) gathers the samples whose 2 x 2 taps touch it
// All arithmetic fp32 (expf, IEEE divisions in the reference's order of operations), the loss sum in fp64.  No atomics: every result
// is a function of the inputs alone, bit for bit.  Coordinates are device data the host cannot check: every kernel clamps them
// into [0, size).
#include "dg_loss_args.h"
#include "dg_device.h"
#include "dg_taps.h"

#define CRFL_SAMPLE_THREADS 64
#define CRFL_PAIR_THREADS 256          // four waves: each takes a quarter of every staged chunk of c
#define CRFL_CC 64                     // samples c staged per chunk
#define CRFL_BWD_THREADS 128

__device__ __forceinline__ int crfl_coord(const int* coords, int i, int size) {
    const int v = coords[i];
    return v < 0 ? 0 : (v > size - 1 ? size - 1 : v);
}

// One thread per (image, sample).  The taps and the blend are F.interpolate's (bilinear, align_corners=False, no antialiasing):
// h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11);  F.normalize: x / max(|x|, eps).
// grid (ceil(n / 64), B), block 64.
__global__ __launch_bounds__(CRFL_SAMPLE_THREADS) void k_crfl_sample(const DgCrflArgs A) {
    const int a = blockIdx.x * CRFL_SAMPLE_THREADS + threadIdx.x, b = blockIdx.y;
    if (a >= A.n) return;
    const int y = crfl_coord(A.coords, a, A.size), x = crfl_coord(A.coords, A.n + a, A.size);
    const size_t row = (size_t)b * A.n + a;
    int y0, y1, x0, x1;
    float ly, lx;
    {   // the guidance: resize(img, size) at (y, x)
        resize_taps(y, A.H, A.size, y0, y1, ly);
        resize_taps(x, A.W, A.size, x0, x1, lx);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const size_t plane = (size_t)A.H * A.W;
        const size_t o00 = (size_t)y0 * A.W + x0, o01 = (size_t)y0 * A.W + x1, o10 = (size_t)y1 * A.W + x0, o11 = (size_t)y1 * A.W + x1;
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* p = A.img + ((size_t)b * 3 + k) * plane;
            v[k] = hy * (hx * p[o00] + lx * p[o01]) + ly * (hx * p[o10] + lx * p[o11]);
        }
        reinterpret_cast<float4*>(A.g4)[row] = make_float4(v[0], v[1], v[2], 0.f);
    }
    // the code vector: resize(code, size) at (y, x), then norm()
    resize_taps(y, A.h, A.size, y0, y1, ly);
    resize_taps(x, A.w, A.size, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const size_t plane = (size_t)A.h * A.w;
    const size_t o00 = (size_t)y0 * A.w + x0, o01 = (size_t)y0 * A.w + x1, o10 = (size_t)y1 * A.w + x0, o11 = (size_t)y1 * A.w + x1;
    float* S = A.S + row * A.Dp;
    double ss = 0.0;                             // the norm in fp64: the stored vector is the correctly rounded unit vector, its own
    for (int d = 0; d < A.D; ++d) {              // norm off 1 by the components' roundings only, not by a rounded divisor
        const float* p = A.code + ((size_t)b * A.D + d) * plane;
        const float v = hy * (hx * p[o00] + lx * p[o01]) + ly * (hx * p[o10] + lx * p[o11]);
        S[d] = v;                                // (this thread reads it back below)
        ss += (double)v * (double)v;
    }
    const double nrm = sqrt(ss);
    const double den = nrm > (double)DG_EPS_NORM ? nrm : (double)DG_EPS_NORM;
    for (int d = 0; d < A.D; ++d) S[d] = (float)((double)S[d] / den);
    for (int d = A.D; d < A.Dp; ++d) S[d] = 0.f;
    A.nrm[row] = (float)nrm;
}

// G = K S of one image, K_ac = w1 exp(-|p_a - p_c|^2 / (2 alpha) - |g_a - g_c|^2 / (2 beta)) + w2 exp(-|p_a - p_c|^2 / (2 gamma)) - shift
// formed in registers and dropped.  A block owns 64 * R rows a (lane = row, R rows per thread: R * 4 * DV accumulators) and walks
// all n samples c in chunks of CRFL_CC staged in LDS (S_c, g_c, p_c: every lane reads the same address, a broadcast); wave k takes
// the k-th quarter of every chunk, so a row's sum is four chains of n / 4 terms, combined through LDS as (w0 + w2) + (w1 + w3).
// DV: float4 per staged row (Dp / 4 <= DV; the columns above Dp stay zero).  Wave 0 then writes G and q_a (fp64) and the block's
// share of the loss sum as one double (the epilogue says how the diagonal and the stored vectors' norms enter).
// CONTRACT with k_crfl_backward, for whoever rewrites this kernel (an MFMA form, say): G_a in the workspace is the sum over c != a -
// the row's own term K_aa S_a only on rows under the eps clamp - and q_a = S_a . G_a / |S_a|^2 in fp64 (0 under the clamp); the loss is
// the estimate for exactly normalised vectors (the diagonal as the constant K_aa, the first-order norm correction), not the loss of
// the stored float32 S.  The issue's plain form (G with the diagonal, q = S . G) has the same mathematics and larger roundings.
// grid (ceil(n / (64 R)), B), block 256, dynamic LDS crfl_pair_lds(DV, R).
template <int DV, int R>
__global__ __launch_bounds__(CRFL_PAIR_THREADS) void k_crfl_pair(const DgCrflArgs A) {
    constexpr int CC = CRFL_CC, CW = CC / 4, ROWS = 64 * R, NIT = (CC * DV + CRFL_PAIR_THREADS - 1) / CRFL_PAIR_THREADS;
    extern __shared__ float4 crfl_smem[];
    float4* sS = crfl_smem;                                  // [CC][DV]
    float4* sg = sS + CC * DV;                               // [CC]
    float2* sp = reinterpret_cast<float2*>(sg + CC);         // [CC] (y, x)
    float4* cb = crfl_smem;                                  // after the walk: [2][DV][ROWS], the waves' partial sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, row0 = blockIdx.x * ROWS, n = A.n, DVp = A.Dp >> 2;
    const float4* gS = reinterpret_cast<const float4*>(A.S) + (size_t)b * n * DVp;
    const float4* gg = reinterpret_cast<const float4*>(A.g4) + (size_t)b * n;

    int ar[R];
    float py[R], px[R];
    float4 ga[R];
    float4 acc[R][DV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int a = row0 + r * 64 + lane;
        ar[r] = a;                                           // (the row's own index: its diagonal term is left out of the walk)
        a = a < n ? a : n - 1;                               // (rows past the end compute a copy of the last one; never written)
        py[r] = (float)crfl_coord(A.coords, a, A.size);
        px[r] = (float)crfl_coord(A.coords, n + a, A.size);
        ga[r] = gg[a];
#pragma unroll
        for (int d = 0; d < DV; ++d) acc[r][d] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = tid; i < CC * DV; i += CRFL_PAIR_THREADS)
        if (i % DV >= DVp) sS[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 pre[NIT], pg = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 pp = make_float2(0.f, 0.f);
    // the chunk's S rows are one contiguous run of floats in the workspace (row stride Dp)
#define CRFL_FETCH(c0)                                                                                            \
    {                                                                                                             \
        const int valid = (n - (c0) < CC ? n - (c0) : CC) * DVp;                                                  \
        _Pragma("unroll") for (int k = 0; k < NIT; ++k) {                                                         \
            const int i = tid + k * CRFL_PAIR_THREADS;                                                            \
            pre[k] = i < valid ? gS[(size_t)(c0) * DVp + i] : make_float4(0.f, 0.f, 0.f, 0.f);                    \
        }                                                                                                         \
        if (tid < CC && (c0) + tid < n) {                                                                         \
            pg = gg[(c0) + tid];                                                                                  \
            pp = make_float2((float)crfl_coord(A.coords, (c0) + tid, A.size), (float)crfl_coord(A.coords, n + (c0) + tid, A.size)); \
        }                                                                                                         \
    }
    CRFL_FETCH(0);
    for (int c0 = 0; c0 < n; c0 += CC) {
        __syncthreads();                                     // the previous chunk has been read
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int i = tid + k * CRFL_PAIR_THREADS;
            if (i < CC * DVp) {
                const int r = i / DVp;
                sS[r * DV + (i - r * DVp)] = pre[k];
            }
        }
        if (tid < CC) { sg[tid] = pg; sp[tid] = pp; }
        __syncthreads();
        if (c0 + CC < n) CRFL_FETCH(c0 + CC);                // in flight under the products below
        const int left = n - c0 - wave * CW;
        const int cend = left < CW ? left : CW;
        for (int cl = 0; cl < cend; ++cl) {
            const int ci = wave * CW + cl;
            const float4 gc = sg[ci];
            const float2 pc = sp[ci];
            float K[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float dy = py[r] - pc.x, dx = px[r] - pc.y;
                const float cd = dy * dy + dx * dx;           // (integers below 2^24: exact)
                const float e0 = ga[r].x - gc.x, e1 = ga[r].y - gc.y, e2 = ga[r].z - gc.z;
                const float gd = e0 * e0 + e1 * e1 + e2 * e2;
                const float k = A.w1 * expf(-cd / A.a2 - gd / A.b2) + A.w2 * expf(-cd / A.g2) - A.shift;
                K[r] = c0 + ci == ar[r] ? 0.f : k;
            }
#pragma unroll
            for (int d = 0; d < DV; ++d) {
                const float4 s = sS[ci * DV + d];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    acc[r][d].x = fmaf(K[r], s.x, acc[r][d].x);
                    acc[r][d].y = fmaf(K[r], s.y, acc[r][d].y);
                    acc[r][d].z = fmaf(K[r], s.z, acc[r][d].z);
                    acc[r][d].w = fmaf(K[r], s.w, acc[r][d].w);
                }
            }
        }
    }
#undef CRFL_FETCH
    // the four waves' chains -> wave 0: (w0 + w2) + (w1 + w3)
#define CRFL_PUT(slot)                                                                                             \
    _Pragma("unroll") for (int r = 0; r < R; ++r) _Pragma("unroll") for (int d = 0; d < DV; ++d)                   \
        cb[((slot) * DV + d) * ROWS + r * 64 + lane] = acc[r][d];
#define CRFL_ADD(slot)                                                                                             \
    _Pragma("unroll") for (int r = 0; r < R; ++r) _Pragma("unroll") for (int d = 0; d < DV; ++d) {                 \
        const float4 t = cb[((slot) * DV + d) * ROWS + r * 64 + lane];                                             \
        acc[r][d].x += t.x; acc[r][d].y += t.y; acc[r][d].z += t.z; acc[r][d].w += t.w;                            \
    }
    __syncthreads();                                         // the staging area becomes the combine buffer
    if (wave >= 2) { CRFL_PUT(wave - 2) }
    __syncthreads();
    if (wave < 2) { CRFL_ADD(wave) }
    __syncthreads();
    if (wave == 1) { CRFL_PUT(0) }
    __syncthreads();
    if (wave != 0) return;
    CRFL_ADD(0)
#undef CRFL_PUT
#undef CRFL_ADD
    // acc = sum over c != a of K_ac S_c.  The diagonal term K_aa S_a . S_a is added here as what it is: K_aa = w1 + w2 - shift times
    // 1 (times |S_a|^2 on a row under the eps clamp).  The stored S_a is a float32 vector, so its norm is 1 + rho_a, not 1: by the
    // symmetry of K the sum over (a, c) of K_ac S_a . S_c / (|S_a| |S_c|) is the sum over a of (1 - 2 rho_a) S_a . G_a to first order.
    const float kaa = A.w1 + A.w2 - A.shift;
    double qsum = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int a = row0 + r * 64 + lane;
        if (a < n) {
            const size_t row = (size_t)b * n + a;
            float4* G = reinterpret_cast<float4*>(A.G) + row * DVp;
            const float4* Sa = gS + (size_t)a * DVp;
            const bool unit = A.nrm[row] >= DG_EPS_NORM;
            double q = 0.0, ss = 0.0;
#pragma unroll
            for (int d = 0; d < DV; ++d) {
                if (d < DVp) {
                    const float4 s = Sa[d];
                    float4 g = acc[r][d];
                    q += (double)s.x * (double)g.x + (double)s.y * (double)g.y + (double)s.z * (double)g.z + (double)s.w * (double)g.w;
                    ss += (double)s.x * (double)s.x + (double)s.y * (double)s.y + (double)s.z * (double)s.z + (double)s.w * (double)s.w;
                    if (!unit) { g.x = fmaf(kaa, s.x, g.x); g.y = fmaf(kaa, s.y, g.y); g.z = fmaf(kaa, s.z, g.z); g.w = fmaf(kaa, s.w, g.w); }
                    G[d] = g;
                }
            }
            // unit rows: q / |S_a|^2 is what the backward projects with (exactly orthogonal to the stored S_a)
            A.q[row] = unit ? q / ss : 0.0;
            qsum += unit ? q * (2.0 / sqrt(ss) - 1.0) + (double)kaa : q + (double)kaa * ss;
        }
    }
    qsum = wave_sum(qsum);
    if (lane == 0) A.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = qsum;
}

// d code (B,D,h,w), every element written.  One block per (image, code pixel): wave 0 walks the n samples - the tap indices and
// weights of the align_corners=False resize are arithmetic on the coordinates - and lists, in sample order, those whose 2 x 2 taps
// touch the pixel (a tap clamped at the border counts twice, as in the forward); then thread d adds weight * dx_a[d] over the list:
//     dx_a = (G_a - S_a q_a) / |x_a|   where |x_a| >= eps,   G_a / eps   otherwise      (the adjoint of norm(), times the factor below)
// with G_a and q_a as k_crfl_pair left them: on a unit row G_a without its own term K_aa S_a, which the projection removes anyway - so
// its rounding, the largest where K is nearly diagonal, never enters - and q_a = S_a . G_a / |S_a|^2 in fp64.
// scaled by -(2 / (B n^2)) * the upstream gradient, read from device memory.
// grid (h * w, B), block 128, dynamic LDS 8 n bytes.
__global__ __launch_bounds__(CRFL_BWD_THREADS) void k_crfl_backward(const DgCrflArgs A) {
    extern __shared__ float4 crfl_bwd_smem[];                 // n ints (the samples), n floats (their weights): all n may touch one pixel
    int* hit_a = reinterpret_cast<int*>(crfl_bwd_smem);
    float* hit_w = reinterpret_cast<float*>(crfl_bwd_smem) + A.n;
    __shared__ int hit_n;
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y, pix = blockIdx.x, n = A.n;
    const int py = pix / A.w, px = pix - py * A.w;
    if (tid < 64) {
        int cnt = 0;
        for (int base = 0; base < n; base += 64) {
            const int a = base + lane;
            float wgt = 0.f;
            if (a < n) {
                int y0, y1, x0, x1;
                float ly, lx;
                resize_taps(crfl_coord(A.coords, a, A.size), A.h, A.size, y0, y1, ly);
                resize_taps(crfl_coord(A.coords, n + a, A.size), A.w, A.size, x0, x1, lx);
                const float wy = (y0 == py ? 1.f - ly : 0.f) + (y1 == py ? ly : 0.f);
                const float wx = (x0 == px ? 1.f - lx : 0.f) + (x1 == px ? lx : 0.f);
                wgt = wy * wx;
            }
            const bool hit = wgt != 0.f;
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
                hit_a[pos] = a;
                hit_w[pos] = wgt;
            }
            cnt += __popcll(m);
        }
        if (lane == 0) hit_n = cnt;
    }
    __syncthreads();
    const int cnt = hit_n;
    const float scale = -2.f / ((float)A.B * (float)n * (float)n) * A.grad_out[0];
    const size_t plane = (size_t)A.h * A.w;
    for (int d = tid; d < A.D; d += CRFL_BWD_THREADS) {
        float acc = 0.f;
        for (int k = 0; k < cnt; ++k) {
            const size_t row = (size_t)b * n + hit_a[k];
            const float g = A.G[row * A.Dp + d], s = A.S[row * A.Dp + d], nr = A.nrm[row];
            const float dx = nr >= DG_EPS_NORM ? (float)((double)g - (double)s * A.q[row]) / nr : g / DG_EPS_NORM;
            acc = fmaf(hit_w[k], dx, acc);
        }
        A.grad_code[((size_t)b * A.D + d) * plane + pix] = scale * acc;
    }
}

static size_t crfl_pair_lds(int DV, int R) {
    const size_t stage = (size_t)(CRFL_CC * DV + CRFL_CC) * 16 + CRFL_CC * 8, comb = (size_t)2 * DV * 64 * R * 16;
    return stage > comb ? stage : comb;
}

template <int DV, int R>
static hipError_t crfl_launch_pair(const DgCrflArgs& A, int* blocks, hipStream_t s) {
    const int lds = (int)crfl_pair_lds(DV, R);
    const dim3 grid((A.n + 64 * R - 1) / (64 * R), A.B);
    *blocks = (int)(grid.x * grid.y);
    return dg_launch_if(lds > 64 * 1024, k_crfl_pair<DV, R>, grid, dim3(CRFL_PAIR_THREADS), lds, s, A);
}

hipError_t dg_launch_crfl_forward(const DgCrflArgs& A, hipStream_t s) {
    hipLaunchKernelGGL(k_crfl_sample, dim3((A.n + CRFL_SAMPLE_THREADS - 1) / CRFL_SAMPLE_THREADS, A.B), dim3(CRFL_SAMPLE_THREADS), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int blocks = 0;
    const int DVp = A.Dp / 4;          // the narrowest instantiation that holds the row: 16, 36, 72 or 128 channels
    if (DVp <= 4) e = crfl_launch_pair<4, 2>(A, &blocks, s);
    else if (DVp <= 9) e = crfl_launch_pair<9, 2>(A, &blocks, s);
    else if (DVp <= 18) e = crfl_launch_pair<18, 2>(A, &blocks, s);
    else e = crfl_launch_pair<32, 1>(A, &blocks, s);
    if (e != hipSuccess) return e;
    const double scale = -1.0 / ((double)A.B * (double)A.n * (double)A.n);
    return dg_launch_loss_reduce(A.part, blocks, scale, A.loss, s);
}

hipError_t dg_launch_crfl_backward(const DgCrflArgs& A, hipStream_t s) {
    hipLaunchKernelGGL(k_crfl_backward, dim3(A.h * A.w, A.B), dim3(CRFL_BWD_THREADS), (size_t)A.n * 8, s, A);
    return hipGetLastError();
}
