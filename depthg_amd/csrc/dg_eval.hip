// The probes' predictions at label resolution and their confusion counts (the producer of the metric):
//   validation_step      src/train_segmentation.py:471-499   interpolate -> linear probe / cluster probe -> arg-max -> metrics.update
//   eval_segmentation    src/eval_segmentation.py:146-170    the same on (code + code_flip.flip(3)) / 2, without the CRF
// Both heads end in an arg-max, and both commute with the bilinear resize:
//   linear:  argmax_k (W interp(x) + b)_k = argmax_k interp(W x + b)_k                   (the tap weights sum to 1)
//   cluster: argmax_k <interp(x) / |interp(x)|, c_k / |c_k|> = argmax_k interp(<x, c_k / |c_k|>)   (|interp(x)| is one positive factor)
// so the code is projected at feature resolution (k_seg_project: B*h*w x D x (n+m), fp32) and only the (n+m)-row score maps are
// resized, per label pixel, right before the arg-maxes (k_seg_score) - nothing at label resolution is written but the predictions
// the caller asks for.  Counts: per-block histograms in LDS (32-bit), one 64-bit atomic per non-empty bin at the end of a
// persistent block (one block per CU); integer sums, so the matrices do not depend on the order.
// Every blend is an explicit fmaf of an explicit product: left to fp-contract, hipcc fuses some lanes of a vector and not others,
// and two identical score rows (duplicated centres or probe rows, a zero code map) would no longer tie exactly.
#include "dg_device.h"
#include "dg_eval_args.h"
#include "dg_seg_rows.h"      // seg_blend_rows, seg_argmax (shared with dg_seg_labels.hip), resize_taps

#include <map>
#include <mutex>

#define SP_THREADS 256        // k_seg_project: positions per block
#define SP_KC 16              // ... score rows per block (a multiple of 4: float4 stores)
#define SS_THREADS 256        // k_seg_score
#define SS_HIST_BYTES (64 * 1024)

// scores[b][q][kp] for q over the h*w grid.  kp < n4: linear row kp (W_kp . x + b_kp); kp >= n4: cluster row kp - n4 (c / |c| . x);
// the padding rows are 0.  x = code[b][:][q], or (code[b][:][i][j] + code_flip[b][:][i][w-1-j]) * 0.5 (the reference's
// (code1 + code2.flip(3)) / 2, the same two fp32 operations).  Block = (256 positions, 16 rows, image); the 16 rows [D][16] in LDS.
template <bool FLIP>
__global__ __launch_bounds__(SP_THREADS) void k_seg_project(const DgSegArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];      // [D][SP_KC]
    const int D = a.D, n = a.n, m = a.m, n4 = (n + 3) / 4 * 4, Kp = dg_seg_kp(n, m), hw = a.h * a.w;
    const int k0 = blockIdx.y * SP_KC, b = blockIdx.z, tid = threadIdx.x;
    for (int i = tid; i < SP_KC * D; i += SP_THREADS) {
        const int r = i / D, d = i - r * D, kp = k0 + r;
        float v = 0.f;
        if (kp < n) v = a.lin_w[(size_t)kp * D + d];
        else if (kp >= n4 && kp - n4 < m) v = a.clusters[(size_t)(kp - n4) * D + d];
        wsm[d * SP_KC + r] = v;
    }
    __syncthreads();
    // F.normalize of the cluster rows: one wave per row, x / max(|x|, eps)
    const int lane = tid & 63;
    for (int r = tid >> 6; r < SP_KC; r += SP_THREADS / 64) {
        const int kp = k0 + r;
        if (kp < n4 || kp - n4 >= m) continue;                       // (wave-uniform)
        float s = 0.f;
        for (int d = lane; d < D; d += 64) { const float v = wsm[d * SP_KC + r]; s = fmaf(v, v, s); }
        s = wave_sum(s);
        const float nrm = fmaxf(sqrtf(s), DG_EPS_NORM_DEFAULT);
        for (int d = lane; d < D; d += 64) wsm[d * SP_KC + r] = wsm[d * SP_KC + r] / nrm;
    }
    __syncthreads();
    const int q = blockIdx.x * SP_THREADS + tid;
    if (q >= hw) return;
    const float* xp = a.code + (size_t)b * D * hw + q;
    const float* fp = a.code_flip;
    if (FLIP) {
        const int i = q / a.w, j = q - i * a.w;
        fp += (size_t)b * D * hw + (size_t)i * a.w + (a.w - 1 - j);
    }
    float acc[SP_KC];
#pragma unroll
    for (int r = 0; r < SP_KC; ++r) acc[r] = 0.f;
    for (int d = 0; d < D; ++d) {
        const float x = FLIP ? (xp[(size_t)d * hw] + fp[(size_t)d * hw]) * 0.5f : xp[(size_t)d * hw];
        const f32x4* wr = reinterpret_cast<const f32x4*>(wsm + d * SP_KC);
#pragma unroll
        for (int r4 = 0; r4 < SP_KC / 4; ++r4) {
            const f32x4 wv = wr[r4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * r4 + j] = fmaf(wv[j], x, acc[4 * r4 + j]);
        }
    }
    float* out = a.scores + ((size_t)b * hw + q) * Kp + k0;
#pragma unroll
    for (int r4 = 0; r4 < SP_KC / 4; ++r4) {
        if (k0 + 4 * r4 >= Kp) break;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kp = k0 + 4 * r4 + j;
            v[j] = kp < n ? acc[4 * r4 + j] + (a.lin_b ? a.lin_b[kp] : 0.f) : acc[4 * r4 + j];
        }
        *reinterpret_cast<f32x4*>(out + 4 * r4) = v;
    }
}

// Persistent blocks over chunks of R consecutive label rows of the flattened (b, Y) space.  Per chunk: the R vertically blended
// score rows [R][w][Kp] go to LDS (coalesced reads of the two source rows), then every pixel of the chunk blends its two columns,
// takes the two arg-maxes, counts and, for images < n_store, writes its predictions.
template <bool LDSHIST>
__global__ __launch_bounds__(SS_THREADS) void k_seg_score(const DgSegArgs a, const int R, const int nchunks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ssm[];
    unsigned int* hist = reinterpret_cast<unsigned int*>(ssm);                 // [2][n][n] (LDSHIST)
    const int n = a.n, m = a.m, n4 = (n + 3) / 4 * 4, Kp = dg_seg_kp(n, m), w = a.w, W = a.W, H = a.H, tid = threadIdx.x;
    const int bins = n * n, wK = w * Kp;
    float* rows = reinterpret_cast<float*>(ssm + (LDSHIST ? ((size_t)2 * bins * 4 + 15) / 16 * 16 : 0));    // [R][w][Kp]
    unsigned long long* gl = reinterpret_cast<unsigned long long*>(a.stats_lin);
    unsigned long long* gc = reinterpret_cast<unsigned long long*>(a.stats_clu);
    if (LDSHIST)
        for (int i = tid; i < 2 * bins; i += SS_THREADS) hist[i] = 0u;
    const long long nrows = (long long)a.B * H;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long long r0 = (long long)c * R;
        const int nr = (int)(nrows - r0 < R ? nrows - r0 : R);
        __syncthreads();                                                       // the previous chunk's readers are done
        seg_blend_rows<SS_THREADS>(a.scores, rows, r0, nr, a.h, H, wK, tid);
        __syncthreads();
        for (int i = tid; i < nr * W; i += SS_THREADS) {
            const int r = i / W, X = i - r * W;
            const long long gr = r0 + r;
            const int b = (int)(gr / H);
            int x0, x1; float lx;
            resize_taps(X, w, W, x0, x1, lx);
            const float* v0 = rows + (size_t)r * wK + x0 * Kp, *v1 = rows + (size_t)r * wK + x1 * Kp;
            const int pl = seg_argmax(v0, v1, lx, n);
            const int pc = seg_argmax(v0 + n4, v1 + n4, lx, m);
            const size_t pix = (size_t)gr * W + X;
            const long long lab = __builtin_nontemporal_load(a.label + pix);
            if (lab >= 0 && lab < n) {                                          // UnsupervisedMetrics.update's mask (src/utils.py:222-232)
                const int bl = pl * n + (int)lab, bc = pc * n + (int)lab;
                if (LDSHIST) {
                    if (gl) atomicAdd(&hist[bl], 1u);
                    if (gc && pc < n) atomicAdd(&hist[bins + bc], 1u);
                } else {
                    if (gl) atomicAdd(&gl[bl], 1ull);
                    if (gc && pc < n) atomicAdd(&gc[bc], 1ull);
                }
            }
            if (b < a.n_store) {
                if (a.preds_lin) a.preds_lin[pix] = pl;
                if (a.preds_clu) a.preds_clu[pix] = pc;
            }
        }
    }
    if (LDSHIST) {
        __syncthreads();
        for (int i = tid; i < 2 * bins; i += SS_THREADS) {
            const unsigned int v = hist[i];
            if (v) atomicAdd(i < bins ? &gl[i] : &gc[i - bins], (unsigned long long)v);   // (a bin is only ever counted with its matrix)
        }
    }
}

// compute units of the current device, asked once per device (also dg_crf.hip)
int dg_cu_count() {
    static std::mutex mu;
    static std::map<int, int> cus;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cus.find(dev);
    if (it != cus.end()) return it->second;
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu < 1) cu = 1;
    cus[dev] = cu;
    return cu;
}

// the score rows at feature resolution into a.scores (also the CRF's eval-route unary, dg_crf.hip)
hipError_t dg_launch_seg_project(const DgSegArgs& a, hipStream_t s) {
    const int hw = a.h * a.w, Kp = dg_seg_kp(a.n, a.m);
    const int psmem = a.D * SP_KC * 4;
    const auto kp = a.code_flip ? k_seg_project<true> : k_seg_project<false>;
    return dg_launch(kp, dim3((hw + SP_THREADS - 1) / SP_THREADS, (Kp + SP_KC - 1) / SP_KC, a.B), dim3(SP_THREADS), psmem, s, a);
}

hipError_t dg_launch_segment_predict(const DgSegArgs& a, hipStream_t s) {
    const int Kp = dg_seg_kp(a.n, a.m);
    hipError_t e = dg_launch_seg_project(a, s);
    if (e != hipSuccess) return e;
    // chunk = R label rows: enough pixels for two passes of the block, as many blended rows as 64 KiB of LDS hold
    const int row_bytes = a.w * Kp * 4;
    int R = (2 * SS_THREADS + a.W - 1) / a.W;
    const int rmax = (64 * 1024) / row_bytes;
    R = R < rmax ? R : rmax;
    R = R < 1 ? 1 : R;
    const long long nrows = (long long)a.B * a.H;
    const long long nchunks = (nrows + R - 1) / R;
    const int cu = dg_cu_count();
    const int blocks = (int)(nchunks < cu ? nchunks : cu);
    const bool ldshist = (size_t)2 * a.n * a.n * 4 <= SS_HIST_BYTES;
    const int smem = (ldshist ? ((2 * a.n * a.n * 4 + 15) / 16 * 16) : 0) + R * row_bytes;
    const auto ks = ldshist ? k_seg_score<true> : k_seg_score<false>;
    return dg_launch(ks, dim3(blocks), dim3(SS_THREADS), smem, s, a, R, (int)nchunks);
}
