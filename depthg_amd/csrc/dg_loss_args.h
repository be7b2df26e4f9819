// The auxiliary loss terms of the training step (dg_crf_loss, dg_aug, dg_rec_loss, dg_loss_reduce .hip; dg_api_loss.hip): constants,
// workspace layouts, argument blocks and launchers.
#pragma once
#include "dg_common.h"
#include "dg_taps.h"        // dg_taps_record_bytes: the augmentation-alignment workspace

// ---- what the three terms share
// A workspace is laid out by one cursor (include/depthg_corr.h describes the layouts to callers): take(bytes) hands out the current
// byte offset and steps over the section to the next multiple of 256; after the last section off is the workspace's size.
struct DgWsCursor {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    }
};
// the section at byte `off` of the workspace at `base`
template <class T>
inline T* dg_ws_at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
// k_loss_reduce: *loss = scale * sum of part[0 .. np - 1], in fp64 and in one fixed order (one block: the same bits on every call)
hipError_t dg_launch_loss_reduce(const double* part, int np, double scale, float* loss, hipStream_t s);

// ---- the contrastive CRF loss term (dg_crf_loss.hip; src/modules.py:1510-1542, src/train_segmentation.py:413-419)
#define DG_CRFL_MAX_D 128
#define DG_CRFL_MAX_N 4096                   // samples per image: k_crfl_backward lists a pixel's samples in LDS (8 bytes each)
#define DG_CRFL_MAX_SIZE 256
#define DG_CRFL_MAX_SIDE 16384               // h, w, H, W: pixel offsets inside one plane stay below 2^28
struct DgCrflWs { size_t S, G, g4, nrm, q, part, total; };
inline DgCrflWs dg_crfl_ws(int B, int D, int n) {
    const size_t rows = (size_t)B * n, Dp = (size_t)(D + 3) / 4 * 4;
    DgWsCursor c;
    DgCrflWs w;
    w.S = c.take(rows * Dp * 4);
    w.G = c.take(rows * Dp * 4);
    w.g4 = c.take(rows * 16);
    w.nrm = c.take(rows * 4);
    w.q = c.take(rows * 8);
    w.part = c.take((size_t)B * ((n + 63) / 64) * 8);      // one double per block of k_crfl_pair, at most
    w.total = c.off;
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
hipError_t dg_launch_crfl_forward(const DgCrflArgs& A, hipStream_t s);      // k_crfl_sample, k_crfl_pair, k_loss_reduce
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
struct DgAugWs { size_t ds, nu, nv, s, part, du, taps, dsd, total; };
inline DgAugWs dg_aug_ws(int B, int D, int h, int w, int n) {
    const size_t rows = (size_t)B * n * n;
    DgWsCursor c;
    DgAugWs ws;
    ws.ds = c.take(rows * 8);
    ws.nu = c.take(rows * 4);
    ws.nv = c.take(rows * 4);
    ws.s = c.take(rows * 4);
    ws.part = c.take((size_t)B * (((size_t)n * n + 63) / 64) * 8);       // one double per block of k_aug_forward
    ws.du = c.take(rows * D * 4);
    ws.taps = c.take((size_t)B * dg_taps_record_bytes(h * w, n * n));
    ws.dsd = c.take(rows * 16);                                          // ds once more, fp64, by position
    ws.total = c.off;
    return ws;
}
// One block for the five kernels; forward: the maps, the forward sections, loss; backward: everything but coord_aug and loss.
struct DgAugArgs {
    const float* code; const float* code_aug; const float* coord_aug;
    float* ds; double* dsd; float* nu; float* nv; float* s; double* part; float* du; char* taps; float* loss;
    const float* grad_out; float* grad_code; float* grad_code_aug;
    int B, D, h, w, n, H, W;
};
hipError_t dg_launch_aug_forward(const DgAugArgs& A, hipStream_t s);        // k_aug_forward, k_loss_reduce
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
struct DgRecWs { size_t ny, nf, s, part, wpart, bpart, total; };
inline DgRecWs dg_rec_ws(int B, int D, int C, int h, int w) {
    const size_t rows = (size_t)B * h * w, S = (size_t)dg_rec_splits(B, C, h, w);
    DgWsCursor c;
    DgRecWs ws;
    ws.ny = c.take(rows * 4);
    ws.nf = c.take(rows * 4);
    ws.s = c.take(rows * 4);
    ws.part = c.take((size_t)B * dg_rec_tiles_per_img(h, w) * 8);        // one double per tile of k_rec_forward
    ws.wpart = c.take(S * C * D * 4);
    ws.bpart = c.take(S * C * 4);
    ws.total = c.off;
    return ws;
}
// One block for the five kernels; forward: the maps, the decoder, ny / nf / s / part, loss; backward: everything but loss (and grad_feats).
struct DgRecArgs {
    const float* code; const float* feats; const float* weight; const float* bias; const float* keep;
    float* ny; float* nf; float* s; double* part; float* wpart; float* bpart; float* loss;
    const float* grad_out; float* grad_code; float* grad_weight; float* grad_bias;
    double inv_n;                            // 1 / (B h w), formed on the host
    float scale;
    int B, D, C, P, tiles_per_img, splits;
    float* grad_feats;                       // d feats (B,C,h,w): dg_launch_rec_backward_feats alone (last: the other fields keep their offsets)
};
hipError_t dg_launch_rec_forward(const DgRecArgs& A, hipStream_t s);        // k_rec_forward, k_loss_reduce
hipError_t dg_launch_rec_backward(const DgRecArgs& A, hipStream_t s);       // k_rec_bwd_code<false>, k_rec_bwd_w, k_rec_combine
// k_rec_bwd_code<true>: d feats too; with grad_code null (then grad_weight and grad_bias are as well) that launch alone, without its
// W^T dy product
hipError_t dg_launch_rec_backward_feats(const DgRecArgs& A, hipStream_t s);
