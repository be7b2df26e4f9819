// The fused depth encoder (dg_depth_enc.hip; dg_api_aux.hip): constants, workspace layout, argument block and launchers.
// The three-stage stack of featurizer.make_depth_downscaling (src/modules.py:497-506):
//     Conv2d(1,64,2,2), LayerNorm2d(64), GELU, Conv2d(64,128,2,2), LayerNorm2d(128), GELU, Conv2d(128,C,2,2)
#pragma once
#include "dg_common.h"

#define DG_DE_TP 32                          // output positions per tile
#define DG_DE_C1 64                          // channels of stage 1
#define DG_DE_C2 128                         // channels of stage 2
#define DG_DE_K2 256                         // stage 2's reduction: 4 children x 64 channels
#define DG_DE_K3 512                         // stage 3's reduction: 4 children x 128 channels
#define DG_DE_MAX_C 768
#define DG_DE_MAX_POS (1 << 24)              // B h w
// the small gradients' partial vector (one per block of k_de_bwd_act), in this order:
// d W1 (64 x 4), d b1, d gamma1, d beta1 (64 each), d b2, d gamma2, d beta2 (128 each)
#define DG_DE_SP 832
#define DG_DE_SP_W1 0
#define DG_DE_SP_B1 256
#define DG_DE_SP_G1 320
#define DG_DE_SP_BE1 384
#define DG_DE_SP_B2 448
#define DG_DE_SP_G2 576
#define DG_DE_SP_BE2 704

inline bool dg_depthenc_supported(int B, int C, int h, int w) {
    return B >= 1 && h >= 1 && w >= 1 && C >= 64 && C <= DG_DE_MAX_C && C % 64 == 0 && (long long)B * h * w <= DG_DE_MAX_POS;
}

// Sections at multiples of 256 bytes.  The forward uses the first two only.
struct DgDepthWs {
    size_t pack_w2, pack_w3, pack_w2t, pack_w3t;     // bf16 fragment-order copies of W2 / W3 and of their transposes
    size_t x2t, da2t;                                // bf16 (tiles, 512, 32) and (tiles, 128, 128): stage-2 activation and its gradient
    size_t part_small, part_w2, part_w3;             // fp32 partial sums of the weight gradients
    size_t total;
    int tiles, blocks_act, splits_w2, splits_w3;
};
inline DgDepthWs dg_depth_ws(int B, int C, int h, int w, bool backward) {
    auto take = [](size_t& off, size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const long long N = (long long)B * h * w;
    DgDepthWs W;
    W.tiles = (int)((N + DG_DE_TP - 1) / DG_DE_TP);
    W.blocks_act = (W.tiles + 1) / 2 > 512 ? 512 : (W.tiles + 1) / 2;
    W.splits_w2 = (W.tiles + 3) / 4 > 64 ? 64 : (W.tiles + 3) / 4;
    W.splits_w3 = (W.tiles + 3) / 4 > 32 ? 32 : (W.tiles + 3) / 4;
    size_t off = 0;
    W.pack_w2 = take(off, (size_t)DG_DE_C2 * DG_DE_K2 * 2);
    W.pack_w3 = take(off, (size_t)C * DG_DE_K3 * 2);
    W.pack_w2t = W.pack_w3t = W.x2t = W.da2t = W.part_small = W.part_w2 = W.part_w3 = off;
    if (backward) {
        W.pack_w2t = take(off, (size_t)DG_DE_C2 * DG_DE_K2 * 2);
        W.pack_w3t = take(off, (size_t)C * DG_DE_K3 * 2);
        W.x2t = take(off, (size_t)W.tiles * DG_DE_K3 * DG_DE_TP * 2);
        W.da2t = take(off, (size_t)W.tiles * DG_DE_K3 * DG_DE_TP * 2);
        W.part_small = take(off, (size_t)W.blocks_act * DG_DE_SP * 4);
        W.part_w2 = take(off, (size_t)W.splits_w2 * DG_DE_C2 * DG_DE_K2 * 4);
        W.part_w3 = take(off, (size_t)W.splits_w3 * ((size_t)C * DG_DE_K3 + 2 * C) * 4);
    }
    W.total = off;
    return W;
}

struct DgDepthEncArgs {
    const float* depth;                      // (B, 8h, 8w)
    const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3;
    const float* residual;                   // forward: (B, C, h, w) or null
    float* out;                              // forward: (B, C, h, w)
    const float* grad_out;                   // backward: (B, C, h, w)
    float *d_w1, *d_b1, *d_g1, *d_be1, *d_w2, *d_b2, *d_g2, *d_be2, *d_w3, *d_b3;
    void *pack_w2, *pack_w3, *pack_w2t, *pack_w3t, *x2t, *da2t;
    float *part_small, *part_w2, *part_w3;
    int B, C, h, w, P, N, tiles, blocks_act, splits_w2, splits_w3;
};

hipError_t dg_launch_depthenc_forward(const DgDepthEncArgs& A, hipStream_t s);
hipError_t dg_launch_depthenc_backward(const DgDepthEncArgs& A, hipStream_t s);
