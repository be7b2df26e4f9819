// Label-free inference (src/demo_segmentation.py:59-78; the CRF route: src/eval_segmentation.py:170-240's label and colour images):
// both probes' byte label maps and painted images, for every image of the batch, without a label tensor and without metrics.
//   k_seg_labels   the label-free sibling of dg_eval.hip's k_seg_score: the same score rows of k_seg_project, the same vertical and
//                  horizontal blends and the same first-maximum arg-max (dg_seg_rows.h) - so its labels are the scored route's bits -
//                  then the cluster id's remap (the Hungarian assignment), the paint, and byte outputs
//   k_label_paint  the same remap and paint on the int64 (G,B,H,W) predictions of dg_dense_crf
// Outputs are bytes: 1 per pixel and label map, 3 per pixel and image.  A lane that stored its own pixel would issue byte stores, three
// of them with a stride of 3 for a colour: instead a chunk's bytes are staged in LDS AT THE 16-BYTE PHASE OF THEIR GLOBAL ADDRESS and
// leave as whole 16-byte vectors; only the at most 15 bytes in front of the first and behind the last vector of a chunk are byte
// stores.  Chunks are disjoint byte ranges, nothing is read back and nothing is atomic: two calls give the same bits.
#include "dg_device.h"
#include "dg_eval_args.h"
#include "dg_seg_rows.h"      // seg_blend_rows, seg_argmax, resize_taps

#define SL_THREADS 256        // k_seg_labels, k_label_paint
#define LP_CHUNK 2048         // k_label_paint: pixels per chunk
#define LP_BLOCKS_PER_CU 8

// where byte 0 of the chunk sits in LDS, per output: its region's start (16-byte aligned) + the phase of its global address
struct SegStage { unsigned char *ll, *lc, *rl, *rc; };
__host__ __device__ inline int seg_stage_1(int cap) { return (cap + 15) / 16 * 16 + 16; }          // a label map's region
__host__ __device__ inline int seg_stage_3(int cap) { return (3 * cap + 15) / 16 * 16 + 16; }      // a colour image's region
__host__ __device__ inline int seg_stage_bytes(int cap) { return 2 * seg_stage_1(cap) + 2 * seg_stage_3(cap); }

__device__ __forceinline__ int seg_phase(const unsigned char* g) { return (int)(reinterpret_cast<uintptr_t>(g) & 15); }

__device__ __forceinline__ SegStage seg_stage(unsigned char* stage, const int cap, const DgPaintArgs& p, const size_t g0) {
    const int s1 = seg_stage_1(cap), s3 = seg_stage_3(cap);
    SegStage st;
    st.ll = stage + seg_phase(p.lab_lin + g0);
    st.lc = stage + s1 + seg_phase(p.lab_clu + g0);
    st.rl = stage + 2 * s1 + seg_phase(p.rgb_lin + 3 * g0);
    st.rc = stage + 2 * s1 + s3 + seg_phase(p.rgb_clu + 3 * g0);
    return st;
}

// the colour table as one dword per row (r | g << 8 | b << 16) and the remap table, in LDS (callers synchronise)
__device__ __forceinline__ void seg_load_tables(const DgPaintArgs& p, unsigned int* cm, int* rm, const int tid) {
    for (int i = tid; i < DG_SEG_MAX_CMAP; i += SL_THREADS) {
        unsigned int c = 0u;
        if (p.cmap && i < p.cmap_rows) c = p.cmap[3 * i] | ((unsigned int)p.cmap[3 * i + 1] << 8) | ((unsigned int)p.cmap[3 * i + 2] << 16);
        cm[i] = c;
        rm[i] = p.remap && i < p.m ? p.remap[i] : i;
    }
}

// the image's pixel as bytes: clamp(rint((v * std + mean) * 255), 0, 255) per channel - UnNormalize's two fp32 roundings
// (src/utils.py:132-136), to_pil_image's scale; the rounding to nearest is the only inexact step.  r | g << 8 | b << 16.
__device__ __forceinline__ unsigned int seg_pixel(const DgPaintArgs& p, const size_t b, const size_t rem) {
    const size_t HW = (size_t)p.H * p.W;
    unsigned int pix = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = __builtin_nontemporal_load(p.img + (b * 3 + c) * HW + rem);
        float f = rintf((dg_mul_rn(v, p.std[c]) + p.mean[c]) * 255.f);
        f = fminf(fmaxf(f, 0.f), 255.f);
        pix |= (unsigned int)(int)f << (8 * c);
    }
    return pix;
}

// (a * cmap[label] + (256 - a) * pix + 128) >> 8 per channel, in integers; a label past the table - 255, "no class", among them -
// paints the table's last row
__device__ __forceinline__ void seg_paint(const unsigned int* cm, const int cmap_rows, const int label, const int a256,
                                          const unsigned int pix, unsigned char* dst3) {
    const unsigned int c = cm[label < cmap_rows ? label : cmap_rows - 1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int cv = (int)((c >> (8 * k)) & 255u), pv = (int)((pix >> (8 * k)) & 255u);
        dst3[k] = (unsigned char)((a256 * cv + (256 - a256) * pv + 128) >> 8);
    }
}

// one pixel's bytes into the stage: i its index in the chunk, (b, rem) its image and its offset in the image, pl / pc the two arg-maxes
__device__ __forceinline__ void seg_emit(const DgPaintArgs& p, const unsigned int* cm, const int* rm, const SegStage& st, const int i,
                                         const size_t b, const size_t rem, const long long pl, const long long pc) {
    const int ll = pl >= 0 && pl < DG_SEG_MAX_LABELS ? (int)pl : 255;
    int lc = 255;
    if (pc >= 0 && pc < p.m) {
        const int t = rm[(int)pc];
        lc = t >= 0 && t < DG_SEG_MAX_LABELS ? t : 255;
    }
    if (p.lab_lin) st.ll[i] = (unsigned char)ll;
    if (p.lab_clu) st.lc[i] = (unsigned char)lc;
    if (p.rgb_lin || p.rgb_clu) {
        const unsigned int pix = p.alpha256 < 256 ? seg_pixel(p, b, rem) : 0u;
        if (p.rgb_lin) seg_paint(cm, p.cmap_rows, ll, p.alpha256, pix, st.rl + 3 * i);
        if (p.rgb_clu) seg_paint(cm, p.cmap_rows, lc, p.alpha256, pix, st.rc + 3 * i);
    }
}

// nbytes staged bytes to g: src holds them at g's 16-byte phase, so every aligned 16-byte vector of the span is one LDS read and one
// store; the bytes in front of the first vector and behind the last go one by one
__device__ __forceinline__ void seg_store_span(const unsigned char* src, unsigned char* g, const int nbytes, const int tid) {
    const int mis = seg_phase(g);
    int head = mis ? 16 - mis : 0;
    head = head < nbytes ? head : nbytes;
    if (tid < head) g[tid] = src[tid];
    const int body = (nbytes - head) >> 4;
    const u32x4* s4 = reinterpret_cast<const u32x4*>(src + head);
    u32x4* g4 = reinterpret_cast<u32x4*>(g + head);
    for (int j = tid; j < body; j += SL_THREADS) g4[j] = s4[j];
    for (int k = head + (body << 4) + tid; k < nbytes; k += SL_THREADS) g[k] = src[k];
}

__device__ __forceinline__ void seg_store_chunk(const DgPaintArgs& p, const SegStage& st, const size_t g0, const int npx, const int tid) {
    if (p.lab_lin) seg_store_span(st.ll, p.lab_lin + g0, npx, tid);
    if (p.lab_clu) seg_store_span(st.lc, p.lab_clu + g0, npx, tid);
    if (p.rgb_lin) seg_store_span(st.rl, p.rgb_lin + 3 * g0, 3 * npx, tid);
    if (p.rgb_clu) seg_store_span(st.rc, p.rgb_clu + 3 * g0, 3 * npx, tid);
}

// Persistent blocks over chunks of R consecutive label rows of the flattened (b, Y) space, as k_seg_score.  Per chunk: the R vertically
// blended score rows to LDS, every pixel's two arg-maxes, remap and paint into the stage, the stage to global memory.  A chunk's pixels
// are one contiguous byte range of every output.  cap = R * W.
__global__ __launch_bounds__(SL_THREADS) void k_seg_labels(const DgSegArgs a, const DgPaintArgs p, const int R, const int nchunks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    __shared__ unsigned int cm[DG_SEG_MAX_CMAP];
    __shared__ int rm[DG_SEG_MAX_CMAP];
    const int n = a.n, m = a.m, n4 = (n + 3) / 4 * 4, Kp = dg_seg_kp(n, m), w = a.w, W = a.W, H = a.H, tid = threadIdx.x;
    const int wK = w * Kp, cap = R * W;
    float* rows = reinterpret_cast<float*>(lsm);                                // [R][w][Kp]
    unsigned char* stage = lsm + (size_t)R * wK * 4;                           // (wK is a multiple of 4: 16-byte aligned)
    seg_load_tables(p, cm, rm, tid);
    const long long nrows = (long long)a.B * H;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long long r0 = (long long)c * R;
        const int nr = (int)(nrows - r0 < R ? nrows - r0 : R);
        __syncthreads();                                                       // the previous chunk's readers are done (first: the tables)
        seg_blend_rows<SL_THREADS>(a.scores, rows, r0, nr, a.h, H, wK, tid);
        const size_t g0 = (size_t)r0 * W;
        const int npx = nr * W;
        const SegStage st = seg_stage(stage, cap, p, g0);
        __syncthreads();
        for (int i = tid; i < npx; i += SL_THREADS) {
            const int r = i / W, X = i - r * W;
            const long long gr = r0 + r;
            const int b = (int)(gr / H), Y = (int)(gr - (long long)b * H);
            int x0, x1; float lx;
            resize_taps(X, w, W, x0, x1, lx);
            const float* v0 = rows + (size_t)r * wK + x0 * Kp, *v1 = rows + (size_t)r * wK + x1 * Kp;
            const int pl = seg_argmax(v0, v1, lx, n);
            const int pc = seg_argmax(v0 + n4, v1 + n4, lx, m);
            seg_emit(p, cm, rm, st, i, (size_t)b, (size_t)Y * W + X, pl, pc);
        }
        __syncthreads();
        seg_store_chunk(p, st, g0, npx, tid);
    }
}

// The CRF route: preds (G,B,H,W) int64, preds[0] the linear probe's and preds[1] the cluster probe's arg-maxes (dg_dense_crf), over
// chunks of LP_CHUNK pixels of the flattened (b, y, x) space.  A value outside [0, 255) is stored as 255.
__global__ __launch_bounds__(SL_THREADS) void k_label_paint(const long long* __restrict__ preds, const int G, const DgPaintArgs p,
                                                            const long long npix, const int nchunks) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[2 * ((LP_CHUNK + 15) / 16 * 16 + 16) + 2 * ((3 * LP_CHUNK + 15) / 16 * 16 + 16)];
    __shared__ unsigned int cm[DG_SEG_MAX_CMAP];
    __shared__ int rm[DG_SEG_MAX_CMAP];
    const int tid = threadIdx.x;
    const size_t HW = (size_t)p.H * p.W;
    seg_load_tables(p, cm, rm, tid);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const size_t g0 = (size_t)c * LP_CHUNK;
        const int npx = (int)((size_t)npix - g0 < LP_CHUNK ? (size_t)npix - g0 : LP_CHUNK);
        const SegStage st = seg_stage(stage, LP_CHUNK, p, g0);
        __syncthreads();                                                       // the previous chunk's readers are done (first: the tables)
        for (int i = tid; i < npx; i += SL_THREADS) {
            const size_t pixel = g0 + i, b = pixel / HW;
            const long long pl = __builtin_nontemporal_load(preds + pixel);
            const long long pc = G > 1 ? __builtin_nontemporal_load(preds + npix + pixel) : -1;
            seg_emit(p, cm, rm, st, i, b, pixel - b * HW, pl, pc);
        }
        __syncthreads();
        seg_store_chunk(p, st, g0, npx, tid);
    }
}

hipError_t dg_launch_segment_labels(const DgSegArgs& a, const DgPaintArgs& p, hipStream_t s) {
    const int Kp = dg_seg_kp(a.n, a.m);
    hipError_t e = dg_launch_seg_project(a, s);
    if (e != hipSuccess) return e;
    // chunk = R label rows, as k_seg_score's: enough pixels for two passes of the block, as many blended rows as 64 KiB of LDS hold,
    // and no more pixels than the stage holds
    const int row_bytes = a.w * Kp * 4;
    int R = (2 * SL_THREADS + a.W - 1) / a.W;
    const int rmax = (64 * 1024) / row_bytes, smax = (DG_SEG_STAGE_BYTES - 128) / (8 * a.W);
    R = R < rmax ? R : rmax;
    R = R < smax ? R : smax;
    R = R < 1 ? 1 : R;
    const long long nrows = (long long)a.B * a.H;
    const long long nchunks = (nrows + R - 1) / R;
    const int cu = dg_cu_count();
    const int blocks = (int)(nchunks < cu ? nchunks : cu);
    const int smem = R * row_bytes + seg_stage_bytes(R * a.W);
    return dg_launch(k_seg_labels, dim3(blocks), dim3(SL_THREADS), smem, s, a, p, R, (int)nchunks);
}

hipError_t dg_launch_label_paint(const int64_t* preds, int G, const DgPaintArgs& p, hipStream_t s) {
    const long long npix = (long long)p.B * p.H * p.W;
    const long long nchunks = (npix + LP_CHUNK - 1) / LP_CHUNK;
    const long long most = (long long)dg_cu_count() * LP_BLOCKS_PER_CU;
    const int blocks = (int)(nchunks < most ? nchunks : most);
    hipLaunchKernelGGL(k_label_paint, dim3(blocks), dim3(SL_THREADS), 0, s, reinterpret_cast<const long long*>(preds), G, p, npix,
                       (int)nchunks);
    return hipGetLastError();
}
