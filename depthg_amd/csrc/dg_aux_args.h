// The stand-alone operations (dg_sample, dg_metrics, dg_knn, dg_lhp, dg_crf_loss, dg_aug, dg_rec_loss, dg_optim, dg_attn, dg_linear .hip; dg_api_aux.hip): constants and launchers.
#pragma once
#include "dg_common.h"
#include "dg_taps.h"        // dg_taps_record_bytes: the augmentation-alignment workspace

hipError_t dg_launch_salience_coords(const float* sal, int B, int H, int W, int n, const float* u_sel, const float* u_fb,
                                     float* out, hipStream_t s);
hipError_t dg_launch_simple_coords(const float* depth, int B, int H, int W, int h, int w, int n, const float* u_val,
                                   const float* u_pick, float* out, hipStream_t s);
hipError_t dg_launch_confusion(const long long* preds, const long long* target, long long count, int ncls, int nrows,
                               unsigned long long* stats, hipStream_t s);
hipError_t dg_launch_sims_nt(const float* q, const float* x, long long rows_q, long long n, int F, long long q_stride, long long x_stride,
                             float* out, long long out_stride, hipStream_t s);
hipError_t dg_launch_topk_rows(const float* vals, long long rows, long long cols, long long row_stride, int k,
                               long long* out_idx, float* out_val, hipStream_t s);
hipError_t dg_launch_lhp_points(const float* depth, int B, int H, int W, int h, int w, float factor, float* points, hipStream_t s);
hipError_t dg_launch_lhp_propagate(bool backward, const float* src, const float* points, float* stats, int B, int D, int P,
                                   float* dst, hipStream_t s);
hipError_t dg_launch_lhp_map(int mode, const float* code, const float* attn, const float* points, const float* divide, int B, int D,
                             int h, int w, int heads, float* out, float* map, hipStream_t s);
hipError_t dg_launch_lhp_map_bwd(int mode, const float* g, const float* map, const float* divide, int B, int D, int h, int w,
                                 float* gcode, hipStream_t s);

// ---- the optimisation step's Adams as one launch (dg_optim.hip; src/train_segmentation.py:447-455, 537-547)
#define DG_ADAM_MAX_SEGS 16                  // segments (tensors) per launch: dg_adam_step splits longer tables
#define DG_ADAM_MAX_GROUPS 16                // hyper-parameter groups per call
#define DG_ADAM_THREADS 256
#define DG_ADAM_CHUNK (4 * DG_ADAM_THREADS)  // elements per block: one 128-bit access per thread and tensor
// at most DG_ADAM_MAX_SEGS segments; tickets: null, or the first segment's counter (segment k takes tickets[k])
hipError_t dg_launch_adam(const dg_adam_seg* segs, int n_seg, const dg_adam_group* groups, int n_groups, bool device_steps,
                          unsigned int* tickets, hipStream_t s);

// ---- the contrastive CRF loss term (dg_crf_loss.hip; src/modules.py:1510-1542, src/train_segmentation.py:413-419)
#define DG_CRFL_MAX_D 128
#define DG_CRFL_MAX_N 4096                   // samples per image: k_crfl_backward lists a pixel's samples in LDS (8 bytes each)
#define DG_CRFL_MAX_SIZE 256
#define DG_CRFL_MAX_SIDE 16384               // h, w, H, W: pixel offsets inside one plane stay below 2^28
// The workspace (include/depthg_corr.h describes it to callers): byte offsets of its sections, each a multiple of 256.
struct DgCrflWs { size_t S, G, g4, nrm, q, part, total; };
inline DgCrflWs dg_crfl_ws(int B, int D, int n) {
    const size_t rows = (size_t)B * n, Dp = (size_t)(D + 3) / 4 * 4;
    auto up256 = [](size_t x) { return (x + 255) / 256 * 256; };
    DgCrflWs w;
    w.S = 0;
    w.G = w.S + up256(rows * Dp * 4);
    w.g4 = w.G + up256(rows * Dp * 4);
    w.nrm = w.g4 + up256(rows * 16);
    w.q = w.nrm + up256(rows * 4);
    w.part = w.q + up256(rows * 8);
    w.total = w.part + up256((size_t)B * ((n + 63) / 64) * 8);      // one double per block of k_crfl_pair, at most
    return w;
}
// One block for the four kernels; forward: everything but grad_*; backward: the workspace sections, coords, sizes and grad_*.
struct DgCrflArgs {
    const float* code; const float* img; const int* coords;
    float* S; float* G; float* g4; float* nrm; double* q; double* part; float* loss;
    const float* grad_out; float* grad_code;
    int B, D, Dp, h, w, H, W, size, n;
    float a2, b2, g2, w1, w2, shift;         // 2 alpha, 2 beta, 2 gamma: the divisors as the reference forms them
};
hipError_t dg_launch_crfl_forward(const DgCrflArgs& A, hipStream_t s);      // k_crfl_sample, k_crfl_pair, k_crfl_reduce
hipError_t dg_launch_crfl_backward(const DgCrflArgs& A, hipStream_t s);     // k_crfl_backward

// ---- the augmentation-alignment loss term (dg_aug.hip; src/train_segmentation.py:400-411)
// The backward's inverse tap records (dg_taps.h) index the n^2 positions with a ushort and are built in one block's LDS: counters and
// offsets over the h w code pixels, four (weight, position) slots per position.
inline size_t dg_aug_taps_lds(int HW, int P) { return (((size_t)(2 * (size_t)HW + 1) * 4 + (size_t)P * 24) + 15) / 16 * 16; }
#define DG_AUG_MAX_LDS (160 * 1024 - 64)     // the workgroup's LDS less build_taps_block's static words
#define DG_AUG_MAX_SIDE 16384                // H, W: offsets inside one coordinate map stay below 2^29
inline bool dg_aug_fits(int h, int w, int n) {
    if (h < 1 || w < 1 || n < 1 || n > 255 || (long long)h * w > (1 << 20)) return false;      // n^2 <= 65025 < 2^16
    return dg_aug_taps_lds(h * w, n * n) <= DG_AUG_MAX_LDS;
}
// The workspace (include/depthg_corr.h describes it to callers): byte offsets of its sections, each a multiple of 256.
struct DgAugWs { size_t ds, nu, nv, s, part, du, taps, dsd, total; };
inline DgAugWs dg_aug_ws(int B, int D, int h, int w, int n) {
    const size_t rows = (size_t)B * n * n;
    auto up256 = [](size_t x) { return (x + 255) / 256 * 256; };
    DgAugWs ws;
    ws.ds = 0;
    ws.nu = ws.ds + up256(rows * 8);
    ws.nv = ws.nu + up256(rows * 4);
    ws.s = ws.nv + up256(rows * 4);
    ws.part = ws.s + up256(rows * 4);
    ws.du = ws.part + up256((size_t)B * (((size_t)n * n + 63) / 64) * 8);       // one double per block of k_aug_forward
    ws.taps = ws.du + up256(rows * D * 4);
    ws.dsd = ws.taps + up256((size_t)B * dg_taps_record_bytes(h * w, n * n));
    ws.total = ws.dsd + up256(rows * 16);                                        // ds once more, fp64, by position
    return ws;
}
// One block for the five kernels; forward: the maps, the forward sections, loss; backward: everything but coord_aug and loss.
struct DgAugArgs {
    const float* code; const float* code_aug; const float* coord_aug;
    float* ds; double* dsd; float* nu; float* nv; float* s; double* part; float* du; char* taps; float* loss;
    const float* grad_out; float* grad_code; float* grad_code_aug;
    int B, D, h, w, n, H, W;
};
hipError_t dg_launch_aug_forward(const DgAugArgs& A, hipStream_t s);        // k_aug_forward, k_aug_reduce
hipError_t dg_launch_aug_backward(const DgAugArgs& A, hipStream_t s);       // k_aug_bwd_pos, k_aug_taps, k_aug_gather

// ---- the reconstruction loss term (dg_rec_loss.hip; src/train_segmentation.py:391-398)
#define DG_REC_MAX_D 128                     // code channels: four 32-row accumulator tiles of d code per position half (the head's own limit)
#define DG_REC_TP 64                         // positions per tile
#define DG_REC_CHUNK 64                      // decoder rows staged in LDS at once
#define DG_REC_BLOCK_TARGET 480              // blocks of the d W kernel: chunks x splits, about two per CU (what the LDS admits)
inline int dg_rec_tiles_per_img(int h, int w) { return (int)(((long long)h * w + DG_REC_TP - 1) / DG_REC_TP); }
// position splits of the d W kernel: each writes one (C, D) partial, summed in fp64 by k_rec_combine
inline int dg_rec_splits(int B, int C, int h, int w) {
    const long long tiles = (long long)B * dg_rec_tiles_per_img(h, w);
    const int chunks = (C + DG_REC_CHUNK - 1) / DG_REC_CHUNK, want = (DG_REC_BLOCK_TARGET + chunks - 1) / chunks;
    return (int)(tiles < want ? tiles : want);
}
// dy chunk [64][65], W chunk [64][D up to a multiple of 8, + 4], code tile [D up to a multiple of 32][65]
inline size_t dg_rec_lds(int D) {
    return ((size_t)DG_REC_CHUNK * 65 + (size_t)DG_REC_CHUNK * (((D + 7) & ~7) + 4) + (size_t)((D + 31) & ~31) * 65) * 4;
}
// sizes the kernels index with int32: positions, tiles, either map's element count and the decoder's
inline bool dg_rec_fits(int B, int D, int C, int h, int w) {
    if (B < 1 || D < 1 || C < 1 || h < 1 || w < 1 || D > DG_REC_MAX_D) return false;
    const long long P = (long long)h * w, big = C > D ? C : D;
    return P <= 0x7fffffffll / B && (long long)B * P <= 0x7fffffffll / big && (long long)C * D + C <= 0x7fffffffll;
}
// The workspace (include/depthg_corr.h describes it to callers): byte offsets of its sections, each a multiple of 256.
struct DgRecWs { size_t ny, nf, s, part, wpart, bpart, total; };
inline DgRecWs dg_rec_ws(int B, int D, int C, int h, int w) {
    const size_t rows = (size_t)B * h * w, S = (size_t)dg_rec_splits(B, C, h, w);
    auto up256 = [](size_t x) { return (x + 255) / 256 * 256; };
    DgRecWs ws;
    ws.ny = 0;
    ws.nf = ws.ny + up256(rows * 4);
    ws.s = ws.nf + up256(rows * 4);
    ws.part = ws.s + up256(rows * 4);
    ws.wpart = ws.part + up256((size_t)B * dg_rec_tiles_per_img(h, w) * 8);     // one double per tile of k_rec_forward
    ws.bpart = ws.wpart + up256(S * C * D * 4);
    ws.total = ws.bpart + up256(S * C * 4);
    return ws;
}
// One block for the five kernels; forward: the maps, the decoder, ny / nf / s / part, loss; backward: everything but loss.
struct DgRecArgs {
    const float* code; const float* feats; const float* weight; const float* bias; const float* keep;
    float* ny; float* nf; float* s; double* part; float* wpart; float* bpart; float* loss;
    const float* grad_out; float* grad_code; float* grad_weight; float* grad_bias;
    double inv_n;                            // 1 / (B h w), formed on the host
    float scale;
    int B, D, C, P, tiles_per_img, splits;
};
hipError_t dg_launch_rec_forward(const DgRecArgs& A, hipStream_t s);        // k_rec_forward, k_rec_reduce
hipError_t dg_launch_rec_backward(const DgRecArgs& A, hipStream_t s);       // k_rec_bwd_code, k_rec_bwd_w, k_rec_combine

// ---- fused attention forward of the frozen ViT (dg_attn.hip; src/dino/vision_transformer.py:80-92)
size_t dg_attn_workspace(int B, int heads, int N);           // bytes of the packed bf16 K / V images
hipError_t dg_launch_attention(const float* qkv, float* out, void* ws, int B, int N, int heads, float scale, hipStream_t s);

// ---- fused bf16 linear layers of the frozen ViT (dg_linear.hip; src/dino/vision_transformer.py:49-65, 68-92, 95-115)
bool dg_linear_supported(int K, int Nout);                   // multiples of 64 up to 3072
size_t dg_linear_packed_bytes(int K, int Nout);              // 0 when unsupported
hipError_t dg_launch_linear_pack(const float* w, int K, int Nout, void* packed, hipStream_t s);
hipError_t dg_launch_linear(const void* x, const float* gamma, const float* beta, float eps, const void* packed, const float* bias,
                            const float* residual, void* out, int M, int K, int Nout, int flags, hipStream_t s);
