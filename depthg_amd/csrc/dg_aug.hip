// The augmentation-alignment loss term of the training step (cfg.aug_alignment_weight; src/train_segmentation.py:400-411):
//     ds   = resize(coord_aug.permute(0,3,1,2), n).permute(0,2,3,1)      (src/utils.py:60-61: bilinear, align_corners=False)
//     u    = sample(code, ds)                                            (src/modules.py:822-825: grid_sample of ds.permute(0,2,1,3),
//                                                                         border, align_corners=True: u[b,:,i,j] reads x = ds[b,j,i,0], y = ds[b,j,i,1])
//     loss = -mean over (b,i,j) of s,   s = <norm(u), norm(code_aug)>    (src/modules.py:789-790: F.normalize(dim=1, eps=1e-10))
// as five kernels, two forward and three backward:
//   k_aug_forward   one thread per position (b,i,j), lanes over neighbouring j: the four resize taps of coord_aug (ds, kept in the
//                   workspace), the four bilinear taps of code, the D-long loop for |u|^2, |v|^2, <u,v>,
//                   then s; |u|, |v|, s to the workspace, the block's sum of -s as one double.  u is never written.
//   k_loss_reduce   the blocks' sums -> the loss scalar (fp64, fixed order; dg_loss_reduce.hip)
//   k_aug_bwd_pos   per position again: u re-formed through its taps, d code_aug written, d u (B,D,n^2) to the workspace
//   k_aug_taps      the sorted inverse tap records of ds, one block per image (build_taps_block, dg_taps.h), their weights from
//                   the fp64 coordinates
//   k_aug_gather    d code, destination-major: every code pixel sums weight * d u over its record list, in position order
// The norm under autograd (what F.normalize's x / clamp_min(|x|, eps) gives in the reference's float32 chain): where |x| >= eps
//     d x = (g - x^ <x^, g>) / |x|,       and where |x| < eps the divisor is the constant eps:   x^ = x / eps,   d x = g / eps
// (no projection: clamp_min passes no gradient to the norm below its bound; at |x| == eps exactly it does).  So a zero vector has
// s = 0 and hands its partner's unit vector, over eps, to its own gradient: large and finite, as in the reference.
// Coordinates and tap weights in fp64 (see aug_resize_taps), all other arithmetic fp32, the loss sum fp64.  No atomics on floating-point data; every result is a function of the inputs alone, bit
// for bit.  Coordinates are device data the host cannot check: aug_pos and dg_taps clamp them into the map (NaN goes to pixel 0).
#include "dg_loss_args.h"
#include "dg_device.h"
#include "dg_taps.h"

#define AUG_POS_THREADS 64             // one wave of positions per block: B * n^2 / 64 blocks spread over the CUs
#define AUG_TAPS_THREADS 256
#define AUG_GATHER_THREADS 256         // lanes over 64 destination pixels, the four waves over the channels

// Coordinates in fp64.  The float32 chain of the reference carries the coordinates' rounding - about 1e-7, times half the map's
// side in the taps' weights - into everything behind them; it is the largest error of the whole term.  The resize of coord_aug,
// the pixel position and the four weights are therefore formed in fp64 from the float32 inputs (a few operations per position) and
// only the weights are rounded to float32.  ds is kept twice: in fp64 by position for the taps, in float32 in the reference's
// layout for build_taps_block, which decides from it WHICH pixels list a position; k_aug_taps then rewrites the records' weights
// from the fp64 copy, so forward, backward and gather use the same weights.
__device__ __forceinline__ void aug_resize_taps(const int dst, const int in, const int out, int& i0, int& i1, double& l1) {
    double src = ((double)dst + 0.5) * ((double)in / (double)out) - 0.5;       // F.interpolate, align_corners=False
    src = src < 0.0 ? 0.0 : src;
    i0 = (int)src; if (i0 > in - 1) i0 = in - 1;
    i1 = i0 < in - 1 ? i0 + 1 : i0;
    l1 = src - (double)i0;
}
// sample()'s pixel position and fractions (grid_sample, border, align_corners=True); NaN goes to pixel 0
struct AugPos { int x0, y0; double fx, fy; };
__device__ __forceinline__ AugPos aug_pos(const double cx, const double cy, int h, int w) {
    double x = ((cx + 1.0) / 2.0) * (double)(w - 1), y = ((cy + 1.0) / 2.0) * (double)(h - 1);
    x = fmin(fmax(x, 0.0), (double)(w - 1));
    y = fmin(fmax(y, 0.0), (double)(h - 1));
    const double x0 = floor(x), y0 = floor(y);
    AugPos q;
    q.x0 = (int)x0; q.y0 = (int)y0; q.fx = x - x0; q.fy = y - y0;
    return q;
}
// The taps of one position on the code map.
struct AugTaps { size_t o00, o01, o10, o11; float w00, w01, w10, w11; };
__device__ __forceinline__ AugTaps aug_taps(const double cx, const double cy, int h, int w) {
    const AugPos q = aug_pos(cx, cy, h, w);
    AugTaps t;
    t.w00 = (float)((1.0 - q.fy) * (1.0 - q.fx)); t.w01 = (float)((1.0 - q.fy) * q.fx);
    t.w10 = (float)(q.fy * (1.0 - q.fx)); t.w11 = (float)(q.fy * q.fx);
    // (a tap past the edge has weight 0 - the coordinate is clamped into the map - and reads the pixel itself instead)
    const size_t pix = (size_t)q.y0 * w + q.x0, dx = q.x0 + 1 <= w - 1 ? 1 : 0, dy = q.y0 + 1 <= h - 1 ? (size_t)w : 0;
    t.o00 = pix; t.o01 = pix + dx; t.o10 = pix + dy; t.o11 = pix + dy + dx;
    return t;
}
// The weight with which the position at (cx, cy) reads pixel (py, px): the sum of its taps that land there.
__device__ __forceinline__ float aug_weight(const double cx, const double cy, int h, int w, int py, int px) {
    const AugPos q = aug_pos(cx, cy, h, w);
    const double wx = (q.x0 == px ? 1.0 - q.fx : 0.0) + (q.x0 + 1 == px ? q.fx : 0.0);
    const double wy = (q.y0 == py ? 1.0 - q.fy : 0.0) + (q.y0 + 1 == py ? q.fy : 0.0);
    return (float)(wy * wx);
}
__device__ __forceinline__ float aug_blend(const float* p, const AugTaps& t) {
    return t.w00 * p[t.o00] + t.w01 * p[t.o01] + t.w10 * p[t.o10] + t.w11 * p[t.o11];
}

// grid (ceil(n^2 / 64), B), block 64.
__global__ __launch_bounds__(AUG_POS_THREADS) void k_aug_forward(const DgAugArgs A) {
    const int n = A.n, P = n * n, p = blockIdx.x * AUG_POS_THREADS + threadIdx.x, b = blockIdx.y;
    double neg = 0.0;
    if (p < P) {
        const int i = p / n, j = p - i * n;
        // ds[b,j,i,:] = resize(coord_aug)[b,:,j,i]: F.interpolate's taps and blend, h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)
        int r0, r1, c0, c1;
        double lr, lc;
        aug_resize_taps(j, A.H, n, r0, r1, lr);
        aug_resize_taps(i, A.W, n, c0, c1, lc);
        const double hr = 1.0 - lr, hc = 1.0 - lc;
        const float* ca = A.coord_aug + (size_t)b * A.H * A.W * 2;
        const size_t q00 = ((size_t)r0 * A.W + c0) * 2, q01 = ((size_t)r0 * A.W + c1) * 2, q10 = ((size_t)r1 * A.W + c0) * 2,
                     q11 = ((size_t)r1 * A.W + c1) * 2;
        double c[2];
#pragma unroll
        for (int k = 0; k < 2; ++k)
            c[k] = hr * (hc * (double)ca[q00 + k] + lc * (double)ca[q01 + k]) + lr * (hc * (double)ca[q10 + k] + lc * (double)ca[q11 + k]);
        float* ds = A.ds + (((size_t)b * n + j) * n + i) * 2;
        ds[0] = (float)c[0]; ds[1] = (float)c[1];
        double* dsd = A.dsd + ((size_t)b * P + p) * 2;
        dsd[0] = c[0]; dsd[1] = c[1];
        const AugTaps t = aug_taps(c[0], c[1], A.h, A.w);
        const size_t plane = (size_t)A.h * A.w;
        const float* pc = A.code + (size_t)b * A.D * plane;
        const float* pv = A.code_aug + (size_t)b * A.D * P + p;
        float uu = 0.f, vv = 0.f, uv = 0.f;
#pragma unroll 4
        for (int d = 0; d < A.D; ++d) {
            const float u = aug_blend(pc, t), v = pv[0];
            uu = fmaf(u, u, uu); vv = fmaf(v, v, vv); uv = fmaf(u, v, uv);
            pc += plane; pv += P;
        }
        const float nu = sqrtf(uu), nv = sqrtf(vv);
        const float s = uv / fmaxf(nu, DG_EPS_NORM) / fmaxf(nv, DG_EPS_NORM);
        const size_t row = (size_t)b * P + p;
        A.nu[row] = nu; A.nv[row] = nv; A.s[row] = s;
        neg = -(double)s;
    }
    neg = wave_sum(neg);
    if (threadIdx.x == 0) A.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = neg;
}

// d code_aug (B,D,n,n), every element written, and d u (B,D,n^2) for the gather.  With c = -(upstream gradient) / (B n^2):
//     d v = c (u^ - s v^) / |v|,   d u = c (v^ - s u^) / |u|      where the norm is >= eps;   c u^ / eps,  c v^ / eps   below it.
// grid (ceil(n^2 / 64), B), block 64.
__global__ __launch_bounds__(AUG_POS_THREADS) void k_aug_bwd_pos(const DgAugArgs A) {
    const int n = A.n, P = n * n, p = blockIdx.x * AUG_POS_THREADS + threadIdx.x, b = blockIdx.y;
    if (p >= P) return;
    const double* dsd = A.dsd + ((size_t)b * P + p) * 2;
    const AugTaps t = aug_taps(dsd[0], dsd[1], A.h, A.w);
    const size_t row = (size_t)b * P + p, plane = (size_t)A.h * A.w;
    const float nu = A.nu[row], nv = A.nv[row], s = A.s[row];
    const bool unit_u = nu >= DG_EPS_NORM, unit_v = nv >= DG_EPS_NORM;
    const float iu = 1.f / fmaxf(nu, DG_EPS_NORM), iv = 1.f / fmaxf(nv, DG_EPS_NORM);
    const float c = -A.grad_out[0] / ((float)A.B * (float)P);
    const float su = unit_u ? s : 0.f, sv = unit_v ? s : 0.f;        // (below eps the divisor is a constant: nothing to project off)
    const float* pc = A.code + (size_t)b * A.D * plane;
    const float* pv = A.code_aug + (size_t)b * A.D * P + p;
    float* gv = A.grad_code_aug + (size_t)b * A.D * P + p;
    float* gu = A.du + (size_t)b * A.D * P + p;
#pragma unroll 4
    for (int d = 0; d < A.D; ++d) {
        const float uh = aug_blend(pc, t) * iu, vh = pv[0] * iv;
        gv[0] = c * (uh - sv * vh) * iv;
        gu[0] = c * (vh - su * uh) * iu;
        pc += plane; pv += P; gv += P; gu += P;
    }
}

// The inverse tap records of ds on the code map: image b's record at taps + b * dg_taps_record_bytes(h w, n^2).
// grid B, block 256, dynamic LDS dg_aug_taps_lds(h w, n^2).
__global__ __launch_bounds__(AUG_TAPS_THREADS) void k_aug_taps(const DgAugArgs A) {
    extern __shared__ float4 aug_taps_smem[];
    DgTapsArgs t;
    t.coords1 = A.ds; t.coords2 = A.ds; t.taps = A.taps;
    t.B = A.B; t.h = A.h; t.w = A.w; t.S = A.n; t.Sh = A.n; t.P = A.n * A.n;
    build_taps_block<AUG_TAPS_THREADS>(t, (int)blockIdx.x, 0, reinterpret_cast<char*>(aug_taps_smem));
    __syncthreads();                                        // the record is in global memory, written by this block
    const int HW = A.h * A.w, P = t.P, b = blockIdx.x;
    char* rec = A.taps + (size_t)b * dg_taps_record_bytes(HW, P);
    const int* off = reinterpret_cast<const int*>(rec);
    float* gw = reinterpret_cast<float*>(rec + (size_t)(HW + 1) * 4);
    const unsigned short* gp = reinterpret_cast<const unsigned short*>(gw + 4 * P);
    const double* dsd = A.dsd + (size_t)b * P * 2;
    for (int q = threadIdx.x; q < HW; q += AUG_TAPS_THREADS) {
        const int py = q / A.w, px = q - py * A.w;
        for (int k = off[q]; k < off[q + 1]; ++k) gw[k] = aug_weight(dsd[2 * gp[k]], dsd[2 * gp[k] + 1], A.h, A.w, py, px);
    }
}

// d code (B,D,h,w), every element written (a pixel no position reads gets 0): the adjoint of sample() as a gather.  Lane = pixel,
// wave k takes the channels k, k + 4, ...; a pixel's list is walked in position order, so the sum has one order.
// grid (ceil(h w / 64), B), block 256.
__global__ __launch_bounds__(AUG_GATHER_THREADS) void k_aug_gather(const DgAugArgs A) {
    const int HW = A.h * A.w, P = A.n * A.n, b = blockIdx.y;
    const int q = blockIdx.x * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
    if (q >= HW) return;
    const char* rec = A.taps + (size_t)b * dg_taps_record_bytes(HW, P);
    const int* off = reinterpret_cast<const int*>(rec);
    const float* gw = reinterpret_cast<const float*>(off + HW + 1);
    const unsigned short* gp = reinterpret_cast<const unsigned short*>(gw + 4 * P);
    const int e0 = off[q], e1 = off[q + 1];
    for (int d = wave; d < A.D; d += AUG_GATHER_THREADS / 64) {
        const float* du = A.du + ((size_t)b * A.D + d) * P;
        float acc = 0.f;
        for (int k = e0; k < e1; ++k) acc = fmaf(gw[k], du[gp[k]], acc);
        A.grad_code[((size_t)b * A.D + d) * HW + q] = acc;
    }
}

hipError_t dg_launch_aug_forward(const DgAugArgs& A, hipStream_t s) {
    const dim3 grid((A.n * A.n + AUG_POS_THREADS - 1) / AUG_POS_THREADS, A.B);
    hipLaunchKernelGGL(k_aug_forward, grid, dim3(AUG_POS_THREADS), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const double scale = 1.0 / ((double)A.B * (double)A.n * (double)A.n);
    return dg_launch_loss_reduce(A.part, (int)(grid.x * grid.y), scale, A.loss, s);
}

hipError_t dg_launch_aug_backward(const DgAugArgs& A, hipStream_t s) {
    const int HW = A.h * A.w, P = A.n * A.n;
    if (!dg_aug_fits(A.h, A.w, A.n)) return hipErrorInvalidValue;       // the records' ushort positions and their LDS image
    const int lds = (int)dg_aug_taps_lds(HW, P);
    if (lds > 64 * 1024) {
        hipError_t e = dg_set_max_smem(reinterpret_cast<const void*>(k_aug_taps), lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_aug_bwd_pos, dim3((P + AUG_POS_THREADS - 1) / AUG_POS_THREADS, A.B), dim3(AUG_POS_THREADS), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_aug_taps, dim3(A.B), dim3(AUG_TAPS_THREADS), lds, s, A);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_aug_gather, dim3((HW + 63) / 64, A.B), dim3(AUG_GATHER_THREADS), 0, s, A);
    return hipGetLastError();
}
