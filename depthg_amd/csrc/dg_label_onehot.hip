// The supervised signal of the correlation loss (cfg.use_true_labels; reference src/train_segmentation.py:219-225 and one_hot_feats,
// src/utils.py:64-65): out (NB, K, H, W) fp32, K = n_classes + 1, channel label + 1 of a pixel 1.0 and every other 0.0, for the
// int64 labels (B, H, W) of the anchors and - one launch, one allocation - of the positives behind them.  The reference's chain forms an
// int64 (B, H, W, K) tensor and a permuted fp32 copy of it; this is a stream that reads each label once and writes each output once.
//   k_label_onehot   blockIdx.y the image, blockIdx.x a span of OH_SPAN pixels of it.  No LDS, no atomics, every element written
//                    exactly once.  Where W % 4 == 0 (a plane is then whole 16-byte vectors from an aligned `out`) a lane owns four
//                    neighbouring pixels: it reads their labels and stores one 16-byte vector per channel plane (a wave writes 1 KB of
//                    every plane in turn).  Any other map goes one pixel per lane and access, lane-contiguous, as the feature cache's
//                    rows do where they meet no 16-byte boundary (dg_feat_cache.hip).
// A label outside [-1, n_classes - 1] selects no channel: its pixel is all zeros (the caller's contract: ops.label_onehot(check=False)).
#include "dg_device.h"
#include "dg_corr_args.h"

#define OH_THREADS 256
#define OH_SPAN (4 * OH_THREADS)        // pixels per block

// the channel of a label, or -1 where it has none
__device__ __forceinline__ int oh_channel(long long label, int K) {
    const long long c = label + 1;
    return (c >= 0 && c < (long long)K) ? (int)c : -1;
}

__global__ __launch_bounds__(OH_THREADS) void k_label_onehot(const long long* __restrict__ label, const long long* __restrict__ label_b, int Ba,
                                                             int K, int HW, int vec, float* __restrict__ out) {
    const int n = blockIdx.y, tid = threadIdx.x;
    const long long* lab = n < Ba ? label + (size_t)n * HW : label_b + (size_t)(n - Ba) * HW;
    float* o = out + (size_t)n * K * HW;
    const int p0 = blockIdx.x * OH_SPAN;
    if (vec) {                                              // (uniform over the launch: no divergence)
        const int p = p0 + 4 * tid;                         // HW % 4 == 0: a quad is inside the map or wholly outside
        if (p >= HW) return;
        int c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = oh_channel(lab[p + u], K);
        for (int k = 0; k < K; ++k)
            *reinterpret_cast<f32x4*>(o + (size_t)k * HW + p) = f32x4{c[0] == k ? 1.f : 0.f, c[1] == k ? 1.f : 0.f, c[2] == k ? 1.f : 0.f,
                                                                      c[3] == k ? 1.f : 0.f};
        return;
    }
    int c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * OH_THREADS + tid;
        c[u] = p < HW ? oh_channel(lab[p], K) : -1;
    }
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + u * OH_THREADS + tid;
            if (p < HW) o[(size_t)k * HW + p] = c[u] == k ? 1.f : 0.f;
        }
    }
}

// (B images in all; the first Ba from `label`, the rest from `label_b`)
hipError_t dg_launch_label_onehot(const int64_t* label, const int64_t* label_b, int Ba, int B, int K, int H, int W, float* out, hipStream_t s) {
    const int HW = H * W;
    const int vec = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    return dg_launch_if(false, k_label_onehot, dim3((HW + OH_SPAN - 1) / OH_SPAN, B), dim3(OH_THREADS), 0, s,
                        reinterpret_cast<const long long*>(label), reinterpret_cast<const long long*>(label_b), Ba, K, HW, vec, out);
}
