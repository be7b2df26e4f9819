// The fused probe step (cfg.dg_fused_probes): both probes of the training step - the linear probe's resized cross entropy
// (src/train_segmentation.py:421-434) and the cluster probe's hard-assignment loss (src/modules.py:647-675, alpha None) - with the
// gradients of their three parameters, for a code that is DETACHED (src/train_segmentation.py:421).  Nothing flows back into the code,
// so d W, d b and d clusters are linear in the two upstream scalars: the forward forms the losses AND the unscaled gradients, the
// backward is one launch that multiplies by the two scalars it reads on the device.
//   k_ps_pos      per 64 positions of an image: the code tile once through LDS; logits W c + b at feature resolution, the cluster probe's
//                 arg-max, 1/|c| and the block's partial loss
//   k_ps_label    per (image, feature row y): the label rows whose upper tap is y; every labelled pixel's softmax ONCE, the adjoint of
//                 the resize along the row through LDS, along the column into two register sums (the rows y and y + 1 it reaches)
//   k_ps_reduce   [d logits ; one-hot(arg) / |c|] x [code ; 1]^T over all positions: d W, d b and the per-centre sums of the normalised
//                 code in one product, split over the positions, one partial per block
//   k_ps_finish   the partials in a fixed order, in double; 1 / count; the centre gradient through the normalisation; the two losses
//   k_ps_scale    (backward) the three gradients = upstream scalar x the forward's unscaled ones
// No floating-point atomics anywhere: every sum has a fixed order, two calls give the same bits.  Every workspace byte that is read
// has been written by an earlier launch of the same call.
#include "dg_device.h"
#include "dg_head_args.h"
#include "dg_taps.h"          // resize_taps

// ---------------------------------------------------------------------------------------------------------------- position pass
// block = 64 positions of one image, 4 waves; wave g takes the 4-row bundles g, g + 4, ... of the stacked matrix [W ; normalised centres]
__global__ __launch_bounds__(256) void k_ps_pos(const DgProbeStepArgs a, const DgProbeStepPlan pl) {
    extern __shared__ float sm[];
    const int D = a.D, n = a.n, m = a.m, P = a.h * a.w, R = n + m, R4 = pl.R4;
    float* M = sm;                              // [R4][D]  (rows R.. are zero)
    float* tile = M + R4 * D;                   // [D][64]
    float* sinv = tile + D * 64;                // [64]
    float* sbest = sinv + 64;                   // [4][64]
    int* sarg = reinterpret_cast<int*>(sbest + 256);   // [4][64]
    const int tid = threadIdx.x, q = tid & 63, g = tid >> 6;
    const int b = blockIdx.x / pl.cpi, p0 = (blockIdx.x - b * pl.cpi) * 64, p = p0 + q;
    for (int i = tid; i < n * D; i += 256) M[i] = a.lin_w[i];
    for (int i = R * D + tid; i < R4 * D; i += 256) M[i] = 0.f;
    for (int c = g; c < m; c += 4) {            // one wave per centre: its norm, then the normalised row
        float s = 0.f;
        for (int d = q; d < D; d += 64) { const float v = a.clusters[(size_t)c * D + d]; s = fmaf(v, v, s); }
        s = wave_sum(s);
        const float inv = 1.f / fmaxf(sqrtf(s), DG_EPS_NORM_DEFAULT);
        for (int d = q; d < D; d += 64) M[(n + c) * D + d] = a.clusters[(size_t)c * D + d] * inv;
    }
    for (int i = tid; i < D * 64; i += 256) {
        const int d = i >> 6, qq = i & 63;
        tile[i] = p0 + qq < P ? a.code[((size_t)b * D + d) * P + p0 + qq] : 0.f;
    }
    __syncthreads();
    if (tid < 64) {
        float s = 0.f;
        for (int d = 0; d < D; ++d) { const float v = tile[d * 64 + tid]; s = fmaf(v, v, s); }
        sinv[tid] = 1.f / fmaxf(sqrtf(s), DG_EPS_NORM_DEFAULT);
    }
    __syncthreads();
    const float inv = sinv[q];
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int r0 = 4 * g; r0 < R; r0 += 16) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* m0 = M + r0 * D;
        for (int d = 0; d < D; ++d) {
            const float t = tile[d * 64 + q];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(m0[i * D + d], t, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + i;
            if (r < n) {
                if (p < P) pl.logits(a.ws)[((size_t)b * n + r) * P + p] = acc[i] + (a.lin_b ? a.lin_b[r] : 0.f);
            } else if (r < R) {
                const float ip = acc[i] * inv;
                if (ip > best) { best = ip; arg = r - n; }           // first maximum wins, as torch.argmax
            }
        }
    }
    sbest[g * 64 + q] = best; sarg[g * 64 + q] = arg;
    __syncthreads();
    if (tid < 64) {
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float v = sbest[k * 64 + q]; const int c = sarg[k * 64 + q];
            if (v > best || (v == best && c < arg)) { best = v; arg = c; }
        }
        if (arg >= m) { arg = 0; best = 0.f; }                       // (no finite similarity: a code that holds NaN)
        float contrib = 0.f;
        if (p < P) {
            pl.inv(a.ws)[(size_t)b * P + p] = inv;
            pl.arg(a.ws)[(size_t)b * P + p] = arg;
            contrib = best;
        }
        contrib = wave_sum(contrib);
        if (tid == 0) pl.part_pos(a.ws)[blockIdx.x] = contrib;
    }
}

// ---------------------------------------------------------------------------------------------------------------- label pass
#define PS_OUT 16            // (class, column) outputs per thread: n * w <= 256 * PS_OUT
// block = (image b, feature row y): the label rows Y whose upper tap y0(Y) is y (they reach the rows y and y1 = min(y + 1, h - 1))
__global__ __launch_bounds__(256) void k_ps_label(const DgProbeStepArgs a, const DgProbeStepPlan pl) {
    extern __shared__ float sm[];
    const int n = a.n, h = a.h, w = a.w, H = a.H, W = a.W, P = h * w;
    float* rows = sm;                           // [2][n][w] the logits of the rows y and y1
    float* dpx = rows + 2 * n * w;              // [n][256] softmax - one-hot of the current 256 pixels
    float* slx = dpx + n * 256;                 // [256] their column weight
    float* red = slx + 256;                     // [8]
    int* band = reinterpret_cast<int*>(red + 8);   // [2] the label rows [band[0], band[1])
    int* start = band + 2;                      // [w + 1] start[x] = the first label column whose left tap is >= x (W: none)
    const int tid = threadIdx.x;
    const int b = blockIdx.x / h, y = blockIdx.x - b * h, y1 = y < h - 1 ? y + 1 : y;
    // the inverse of the two tap maps, once: every entry has one writer
    if (tid < 2) band[tid] = 0;
    for (int x = tid; x <= w; x += 256) start[x] = W;
    __syncthreads();
    for (int Y = tid; Y < H; Y += 256) {
        int i0, i1, j0 = -1, j1; float l;
        resize_taps(Y, h, H, i0, i1, l);
        if (i0 != y) continue;
        if (Y > 0) resize_taps(Y - 1, h, H, j0, j1, l);
        if (j0 != y) band[0] = Y;
        j0 = -1;
        if (Y < H - 1) resize_taps(Y + 1, h, H, j0, j1, l);
        if (j0 != y) band[1] = Y + 1;
    }
    for (int X = tid; X < W; X += 256) {
        int i0, i1, j0 = -1, j1; float l;
        resize_taps(X, w, W, i0, i1, l);
        if (X > 0) resize_taps(X - 1, w, W, j0, j1, l);
        for (int x = j0 + 1; x <= i0; ++x) start[x] = X;
    }
    for (int i = tid; i < 2 * n * w; i += 256) {
        const int r = i / (n * w), j = i - r * n * w;
        rows[i] = pl.logits(a.ws)[(size_t)b * n * P + (size_t)(j / w) * P + (r ? y1 : y) * w + j % w];
    }
    // this thread's outputs o = tid + 256 j -> (class, column), fixed for the whole block
    const int nout = n * w;
    int okx[PS_OUT];
    float top[PS_OUT], bot[PS_OUT];
#pragma unroll
    for (int j = 0; j < PS_OUT; ++j) {
        const int o = tid + 256 * j, k = o / w;
        okx[j] = o < nout ? (k << 16) | (o - k * w) : -1;
        top[j] = bot[j] = 0.f;
    }
    __syncthreads();
    const int Y0 = band[0], Y1 = band[1];
    float lsum = 0.f;
    int cnt = 0;
    for (int Y = Y0; Y < Y1; ++Y) {
        int t0, t1; float ly;
        resize_taps(Y, h, H, t0, t1, ly);
        for (int X0 = 0; X0 < W; X0 += 256) {
            __syncthreads();                                          // (the gather of the previous pixels is over)
            const int X = X0 + tid;
            if (X < W) {
                int x0, x1; float lx;
                resize_taps(X, w, W, x0, x1, lx);
                slx[tid] = lx;
                const int64_t lab = a.label[((size_t)b * H + Y) * W + X];
                if (lab >= 0 && lab < n) {
                    auto val = [&](const int c) {
                        const float* r0 = rows + c * w, *r1 = rows + (n + c) * w;
                        return (1.f - ly) * (r0[x0] * (1.f - lx) + r0[x1] * lx) + ly * (r1[x0] * (1.f - lx) + r1[x1] * lx);
                    };
                    float mx = -INFINITY, z = 0.f;
                    for (int c = 0; c < n; ++c) mx = fmaxf(mx, val(c));
                    for (int c = 0; c < n; ++c) { const float e = expf(val(c) - mx); z += e; dpx[c * 256 + tid] = e; }
                    const float iz = 1.f / z;
                    for (int c = 0; c < n; ++c) dpx[c * 256 + tid] = dpx[c * 256 + tid] * iz - (c == (int)lab ? 1.f : 0.f);
                    lsum += logf(z) + mx - val((int)lab);
                    cnt += 1;
                } else {
                    for (int c = 0; c < n; ++c) dpx[c * 256 + tid] = 0.f;
                }
            }
            __syncthreads();
            const int Xe = min(X0 + 256, W);
#pragma unroll
            for (int j = 0; j < PS_OUT; ++j) {
                if (okx[j] < 0) continue;
                const int k = okx[j] >> 16, x = okx[j] & 0xffff;
                const float* dk = dpx + k * 256 - X0;
                float s = 0.f;
                // pixels whose left tap is x (their right tap too where x is the last column), then those whose right tap is x
                const int lo = max(start[x], X0), hi = min(start[x + 1], Xe);
                if (x == w - 1) { for (int Xp = lo; Xp < hi; ++Xp) s += dk[Xp]; }
                else { for (int Xp = lo; Xp < hi; ++Xp) s = fmaf(dk[Xp], 1.f - slx[Xp - X0], s); }
                if (x > 0) {
                    const int lo1 = max(start[x - 1], X0), hi1 = min(start[x], Xe);
                    for (int Xp = lo1; Xp < hi1; ++Xp) s = fmaf(dk[Xp], slx[Xp - X0], s);
                }
                top[j] = fmaf(1.f - ly, s, top[j]);
                bot[j] = fmaf(ly, s, bot[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PS_OUT; ++j) {
        if (okx[j] < 0) continue;
        const int k = okx[j] >> 16, x = okx[j] & 0xffff;
        const size_t o = ((size_t)b * n + k) * P + (size_t)y * w + x;
        pl.ptop(a.ws)[o] = top[j];
        pl.pbot(a.ws)[o] = bot[j];
    }
    lsum = wave_sum(lsum);
    float fc = wave_sum((float)cnt);                                  // (a block sees fewer than 2^24 pixels: exact)
    if ((tid & 63) == 0) { red[tid >> 6] = lsum; red[4 + (tid >> 6)] = fc; }
    __syncthreads();
    if (tid == 0) {
        pl.part_lab(a.ws)[2 * blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        reinterpret_cast<int*>(pl.part_lab(a.ws))[2 * blockIdx.x + 1] = (int)(red[4] + red[5] + red[6] + red[7]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- reduction pass
#define PS_KC 64             // positions per chunk
#define PS_LD 65             // its LDS rows (odd: lanes on consecutive rows hit consecutive banks)
#define PS_TILES 5           // 4 x 4 output tiles per thread: (R4 / 4) * (DC4 / 4) <= 32 * 33
// block s of pl.splits walks the chunks s, s + splits, ...; thread tile (tr, td) owns the rows tr + TR i and the columns td + TD j
__global__ __launch_bounds__(256) void k_ps_reduce(const DgProbeStepArgs a, const DgProbeStepPlan pl) {
    extern __shared__ float sm[];
    const int D = a.D, n = a.n, m = a.m, h = a.h, w = a.w, P = h * w, R = n + m, DC = D + 1;
    const int R4 = pl.R4, DC4 = pl.DC4, TR = R4 / 4, TD = DC4 / 4, ntiles = TR * TD;
    float* G = sm;                              // [R4][PS_LD]  d logits, then one-hot(arg) / |c|
    float* C = G + R4 * PS_LD;                  // [DC4][PS_LD] the code, then a row of ones (its column sums d b)
    const int tid = threadIdx.x;
    double acc[PS_TILES][16];                   // (products of two floats are exact in double: the chunk walk adds no rounding of its own)
#pragma unroll
    for (int t = 0; t < PS_TILES; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0;
    for (int ch = blockIdx.x; ch < pl.chunks; ch += pl.splits) {
        const int b = ch / pl.cpi, p0 = (ch - b * pl.cpi) * PS_KC;
        __syncthreads();
        for (int i = tid; i < R4 * PS_KC; i += 256) {
            const int r = i >> 6, q = i & 63, p = p0 + q;
            float v = 0.f;
            if (p < P) {
                if (r < n) {
                    const int y = p / w;
                    const size_t o = ((size_t)b * n + r) * P + p;
                    v = pl.ptop(a.ws)[o];
                    if (y >= 1) v += pl.pbot(a.ws)[o - w];
                    if (y == h - 1) v += pl.pbot(a.ws)[o];
                } else if (r < R) {
                    v = pl.arg(a.ws)[(size_t)b * P + p] == r - n ? pl.inv(a.ws)[(size_t)b * P + p] : 0.f;
                }
            }
            G[r * PS_LD + q] = v;
        }
        for (int i = tid; i < DC4 * PS_KC; i += 256) {
            const int d = i >> 6, q = i & 63, p = p0 + q;
            float v = 0.f;
            if (p < P) v = d < D ? a.code[((size_t)b * D + d) * P + p] : (d == D ? 1.f : 0.f);
            C[d * PS_LD + q] = v;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < PS_TILES; ++t) {
            const int tile = tid + 256 * t;
            if (tile >= ntiles) continue;
            const int tr = tile / TD, td = tile - tr * TD;
            const float* g0 = G + tr * PS_LD, *c0 = C + td * PS_LD;
#pragma unroll 4
            for (int k = 0; k < PS_KC; ++k) {
                double gv[4], cv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { gv[i] = g0[i * TR * PS_LD + k]; cv[i] = c0[i * TD * PS_LD + k]; }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[t][i * 4 + j] = fma(gv[i], cv[j], acc[t][i * 4 + j]);
            }
        }
    }
    double* out = pl.part_red(a.ws) + (size_t)blockIdx.x * R * DC;
#pragma unroll
    for (int t = 0; t < PS_TILES; ++t) {
        const int tile = tid + 256 * t;
        if (tile >= ntiles) continue;
        const int tr = tile / TD, td = tile - tr * TD;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = tr + TR * i, d = td + TD * j;
                if (r < R && d < DC) out[r * DC + d] = acc[t][i * 4 + j];
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- finish
// blocks 0 .. R - 1: one row of the stacked product (a class of the linear probe, or a centre); block R: the two losses.  The partial
// sums of the label pass are float, the reduction pass's are double; from here on the arithmetic is double, so that the backward's product with the upstream scalar is the one rounding
// between the partial sums and the gradient (the unfused chain scales by upstream / count BEFORE its sums: it rounds once too).
__global__ __launch_bounds__(256) void k_ps_finish(const DgProbeStepArgs a, const DgProbeStepPlan pl) {
    __shared__ double red[4][132];
    __shared__ double tot[132];
    __shared__ double w2[4];
    __shared__ long long wc[4];
    const int D = a.D, n = a.n, P = a.h * a.w, R = n + a.m, DC = D + 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = blockIdx.x;
    const int nlab = a.B * a.h;
    // the labelled pixels of the batch (integers: any order gives the same sum)
    long long c = 0;
    for (int i = tid; i < nlab; i += 256) c += reinterpret_cast<const int*>(pl.part_lab(a.ws))[2 * i + 1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) wc[wv] = c;
    __syncthreads();
    const double count = (double)(wc[0] + wc[1] + wc[2] + wc[3]);
    const double sc = -1.0 / ((double)a.B * (double)P);
    if (r == R) {
        double s = 0.0, s2 = 0.0;
        for (int i = tid; i < nlab; i += 256) s += (double)pl.part_lab(a.ws)[2 * i];
        for (int i = tid; i < pl.chunks; i += 256) s2 += (double)pl.part_pos(a.ws)[i];
        s = wave_sum(s); s2 = wave_sum(s2);
        if (lane == 0) { red[0][wv] = s; red[1][wv] = s2; }
        __syncthreads();
        if (tid == 0) {
            a.out3[0] = (float)(((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / count);       // (no labelled pixel: 0 / 0)
            a.out3[1] = (float)(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) * sc);
            a.out3[2] = (float)count;
        }
        return;
    }
    // the row's partial sums: wave wv adds the splits wv, wv + 4, ..., then the four in order
    for (int d = lane; d < DC; d += 64) {
        double s = 0.0;
        for (int k = wv; k < pl.splits; k += 4) s += pl.part_red(a.ws)[((size_t)k * R + r) * DC + d];
        red[wv][d] = s;
    }
    __syncthreads();
    for (int d = tid; d < DC; d += 256) tot[d] = (red[0][d] + red[1][d]) + (red[2][d] + red[3][d]);
    __syncthreads();
    double* grads = pl.grads(a.ws);             // [n][D] d W, [n] d b, [m][D] d clusters - for upstream gradients of 1
    if (r < n) {
        const double ic = 1.0 / count;          // (no labelled pixel: 1 / 0, and the gradient 0 x inf = NaN, as the loss 0 / 0)
        for (int d = tid; d < D; d += 256) grads[r * D + d] = tot[d] * ic;
        if (tid == 0) grads[n * D + r] = tot[D] * ic;
        return;
    }
    // centre cc: g = -(1 / (B P)) sum of the normalised codes it won; d clusters = (g - nc <nc, g>) / |c|   (|c| above eps)
    const int cc = r - n;
    double v = 0.0, g = 0.0;
    if (tid < D) { v = (double)a.clusters[(size_t)cc * D + tid]; g = tot[tid] * sc; }
    double s = wave_sum(v * v);
    if (lane == 0) w2[wv] = s;
    __syncthreads();
    const double raw = sqrt((w2[0] + w2[1]) + (w2[2] + w2[3])), nrm = fmax(raw, (double)DG_EPS_NORM_DEFAULT);
    __syncthreads();
    s = wave_sum(g * (v / nrm));
    if (lane == 0) w2[wv] = s;
    __syncthreads();
    const double dot = (w2[0] + w2[1]) + (w2[2] + w2[3]);
    if (tid < D) grads[n * D + n + cc * D + tid] = raw < (double)DG_EPS_NORM_DEFAULT ? g / nrm : (g - (v / nrm) * dot) / nrm;
}

// ---------------------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(256) void k_ps_scale(const double* __restrict__ grads, const float* __restrict__ g_lin, const float* __restrict__ g_clu,
                                                  int nw, int nb, int nc, float* __restrict__ gw, float* __restrict__ gb, float* __restrict__ gc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nw) gw[i] = (float)((double)g_lin[0] * grads[i]);
    else if (i < nw + nb) gb[i - nw] = (float)((double)g_lin[0] * grads[i]);
    else if (i < nw + nb + nc) gc[i - nw - nb] = (float)((double)g_clu[0] * grads[i]);
}

// ---------------------------------------------------------------------------------------------------------------- host
// The plan of a shape: what is refused (with the reason), the workspace's sections and the launches' LDS - decided once, in front of
// any launch.  Returns null when the shape is served, else the reason.
const char* dg_probe_step_plan(int B, int D, int n, int m, int h, int w, int H, int W, DgProbeStepPlan& pl) {
    if (D > 128) return "the fused probe step needs D <= 128";
    if (n > 64 || m > 64) return "the fused probe step needs n_lin <= 64 and n_clu <= 64";
    if ((long long)n * w > 256 * PS_OUT) return "the fused probe step needs n_lin * w <= 4096 (the label pass's register sums)";
    if ((long long)B * h * w > (1 << 24) || (long long)H * W > (1LL << 30) || (long long)B * h > (1 << 24))
        return "the fused probe step needs B*h*w <= 2^24 and H*W <= 2^30";
    const int P = h * w, R = n + m, DC = D + 1;
    pl.R4 = (R + 3) / 4 * 4; pl.DC4 = (DC + 3) / 4 * 4;
    pl.cpi = (P + PS_KC - 1) / PS_KC; pl.chunks = B * pl.cpi; pl.splits = pl.chunks < 256 ? pl.chunks : 256;
    pl.smem_pos = (pl.R4 * D + D * 64 + 64 + 512) * 4;
    pl.smem_label = (2 * n * w + n * 256 + 256 + 8 + 2 + w + 1) * 4;
    pl.smem_reduce = (pl.R4 + pl.DC4) * PS_LD * 4;
    if (pl.smem_pos > 160 * 1024 || pl.smem_label > 160 * 1024 || pl.smem_reduce > 160 * 1024) return "the fused probe step's tiles do not fit the LDS";
    auto sec = [](size_t& at, size_t floats) { const size_t o = at; at += (floats + 3) / 4 * 4; return o; };
    size_t at = 0;
    const size_t BnP = (size_t)B * n * P, BP = (size_t)B * P;
    pl.o_logits = sec(at, BnP); pl.o_ptop = sec(at, BnP); pl.o_pbot = sec(at, BnP);
    pl.o_inv = sec(at, BP); pl.o_arg = sec(at, BP);
    pl.o_part_pos = sec(at, pl.chunks); pl.o_part_lab = sec(at, (size_t)2 * B * h);
    pl.o_part_red = sec(at, 2 * (size_t)pl.splits * R * DC);                  // (doubles)
    pl.o_grads = sec(at, 2 * ((size_t)n * D + n + (size_t)m * D));      // (doubles)
    pl.floats = at;
    return nullptr;
}

hipError_t dg_launch_probe_step_fwd(const DgProbeStepArgs& a, const DgProbeStepPlan& pl, hipStream_t s) {
    hipError_t e = dg_launch(k_ps_pos, dim3(pl.chunks), dim3(256), pl.smem_pos, s, a, pl);
    if (e != hipSuccess) return e;
    e = dg_launch(k_ps_label, dim3(a.B * a.h), dim3(256), pl.smem_label, s, a, pl);
    if (e != hipSuccess) return e;
    e = dg_launch(k_ps_reduce, dim3(pl.splits), dim3(256), pl.smem_reduce, s, a, pl);
    if (e != hipSuccess) return e;
    return dg_launch_if(false, k_ps_finish, dim3(a.n + a.m + 1), dim3(256), 0, s, a, pl);
}

hipError_t dg_launch_probe_step_bwd(const float* ws, const DgProbeStepPlan& pl, const float* g_lin, const float* g_clu, int D, int n, int m,
                                    float* gw, float* gb, float* gc, hipStream_t s) {
    const int total = n * D + n + m * D;
    return dg_launch_if(false, k_ps_scale, dim3((total + 255) / 256), dim3(256), 0, s, pl.grads(const_cast<float*>(ws)), g_lin, g_clu,
                        n * D, n, m * D, gw, gb, gc);
}
