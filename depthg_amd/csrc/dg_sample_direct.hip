// sample() (src/modules.py:822-825: grid_sample, bilinear, padding_mode='border', align_corners=True, coordinates transposed) of NCHW
// fp32 maps into rows [image][position][Kout], the four taps of every (position, channel) read IN PLACE: no channel-last copy of the
// maps (k_nchw_to_nhwc + k_gather_rows) and no LDS planes (k_plane_sample).  The loss samples S x S points per image; on a map of the
// labels' resolution (cfg.use_true_labels: 224 x 224 x 28 channels x 32 images = 180 MB per map) the copies move 360 MB each way to
// serve 7 x 32 x 121 = 27 104 positions that touch 3 M of the maps' 90 M elements.
//   k_sample_direct  one block = 8 positions of one (job, image); the 32 lanes of a position walk the channels one at a time.  Channel k
//                    of a tap is map[(img * K + k) * h * w + pix] - offsets in 64 bits (B K h w passes 2^31 at the limits).  The loads
//                    are scattered by construction (one 4-byte element per tap and channel: latency-bound, served by L2 and the
//                    Infinity Cache where positions share lines); the stores are not: a position's row is contiguous and its lanes
//                    write it 32 channels at a time (128 bytes fp32, 64 bytes bf16).  No LDS, no atomics; every element of every row
//                    - the zero padding K..Kout-1 included - is written exactly once.
// Tap arithmetic as in k_gather_rows (dg_small.hip) / k_plane_sample / k_gather_norm: the same operations in the same order.
// A batch-map entry outside [0, B) is the caller's error; it is clamped, so that no read leaves the maps.
#include "dg_device.h"
#include "dg_corr_args.h"

__global__ __launch_bounds__(256) void k_sample_direct(const DgSampleDirectArgs a) {
    const int job = blockIdx.z, n = blockIdx.y, p = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    if (p >= a.P) return;
    const int K = a.K[job], hh = a.h[job], ww = a.w[job];
    const int ii = p / a.S, j = p - ii * a.S;
    const float* cc = a.coords[job] + (((size_t)n * a.S + j) * a.Sh + ii) * 2;
    float x = ((cc[0] + 1.f) / 2.f) * (float)(ww - 1);
    float y = ((cc[1] + 1.f) / 2.f) * (float)(hh - 1);
    x = fminf(fmaxf(x, 0.f), (float)(ww - 1));
    y = fminf(fmaxf(y, 0.f), (float)(hh - 1));
    const float x0f = floorf(x), y0f = floorf(y);
    const float wx1 = x - x0f, wy1 = y - y0f, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const bool inx = x0 + 1 <= ww - 1, iny = y0 + 1 <= hh - 1;
    const float w00 = wy0 * wx0, w01 = inx ? wy0 * wx1 : 0.f, w10 = iny ? wy1 * wx0 : 0.f, w11 = (inx && iny) ? wy1 * wx1 : 0.f;
    const int pix = y0 * ww + x0, dx = inx ? 1 : 0, dy = iny ? ww : 0;
    int img = a.srcidx[job] ? (int)a.srcidx[job][n] : n;
    img = min(max(img, 0), a.B - 1);
    const size_t HW = (size_t)hh * ww;
    const float* __restrict__ t00 = a.src[job] + (size_t)img * K * HW + pix;      // channel 0 of the four taps; channel k lies k * HW further
    const float* __restrict__ t01 = t00 + dx;
    const float* __restrict__ t10 = t00 + dy;
    const float* __restrict__ t11 = t00 + dy + dx;
    const int Kout = a.Kout[job];
    const bool as16 = a.as_bf16[job] != 0;
    float* __restrict__ out = static_cast<float*>(a.rows[job]) + ((size_t)n * a.P + p) * Kout;
    __bf16* __restrict__ out16 = static_cast<__bf16*>(a.rows[job]) + ((size_t)n * a.P + p) * Kout;
    for (int k = l; k < Kout; k += 32) {
        float acc = 0.f;
        if (k < K) {
            const size_t o = (size_t)k * HW;
            const float a0 = t00[o], a1 = t01[o], a2 = t10[o], a3 = t11[o];
            acc = a0 * w00;
            acc = fmaf(a1, w01, acc);
            acc = fmaf(a2, w10, acc);
            acc = fmaf(a3, w11, acc);
        }
        if (as16) out16[k] = (__bf16)acc;
        else out[k] = acc;
    }
}

hipError_t dg_launch_sample_direct(const DgSampleDirectArgs& a, hipStream_t s) {
    if (a.njobs < 1) return hipSuccess;
    hipLaunchKernelGGL(k_sample_direct, dim3((a.P + 7) / 8, a.B, a.njobs), dim3(256), 0, s, a);
    return hipGetLastError();
}
