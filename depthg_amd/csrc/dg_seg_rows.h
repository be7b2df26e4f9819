// What the kernels that resize the probes' score rows per label pixel share (dg_eval.hip: k_seg_score; dg_seg_labels.hip: k_seg_labels):
// the vertical blend of a chunk of label rows into LDS and the horizontal blend with its first-maximum arg-max.  One statement of each:
// the label-free route gives the scored route's bits because it runs the scored route's arithmetic.
// Every blend is an explicit fmaf of an explicit product (dg_eval.hip's header says why).
#pragma once
#include "dg_device.h"
#include "dg_taps.h"          // resize_taps

// rows[r][x][kp] for r < nr: the score rows of label rows r0 + r of the flattened (b, Y) space, blended between their two source rows
// (coalesced float4 reads of both).  scores (B, h, w*Kp); wK = w * Kp, a multiple of 4.  NT threads, all of them call.
template <int NT>
__device__ __forceinline__ void seg_blend_rows(const float* __restrict__ scores, float* rows, const long long r0, const int nr, const int h,
                                               const int H, const int wK, const int tid) {
    for (int r = 0; r < nr; ++r) {
        const int b = (int)((r0 + r) / H), Y = (int)(r0 + r - (long long)b * H);
        int y0, y1; float ly;
        resize_taps(Y, h, H, y0, y1, ly);
        const float* s0 = scores + ((size_t)b * h + y0) * wK;
        const float* s1 = scores + ((size_t)b * h + y1) * wK;
        float* dst = rows + (size_t)r * wK;
        for (int e = tid * 4; e < wK; e += NT * 4) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(s0 + e), v = *reinterpret_cast<const f32x4*>(s1 + e);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaf(v[j], ly, u[j] * (1.f - ly));
            *reinterpret_cast<f32x4*>(dst + e) = o;
        }
    }
}

// arg-max of interp(scores) over rows [0, cnt) of a part, first maximum wins (torch.argmax)
__device__ __forceinline__ int seg_argmax(const float* __restrict__ v0, const float* __restrict__ v1, const float lx, const int cnt) {
    float best = -INFINITY;
    int arg = 0;
    for (int k4 = 0; k4 < cnt; k4 += 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(v0 + k4), c = *reinterpret_cast<const f32x4*>(v1 + k4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = fmaf(c[j], lx, a[j] * (1.f - lx));
            if (k4 + j < cnt && v > best) { best = v; arg = k4 + j; }
        }
    }
    return arg;
}
