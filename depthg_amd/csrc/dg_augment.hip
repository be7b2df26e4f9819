// GPU batch augmentation (depthg_amd/augment.py): the dataset's augmented view and its coordinate map, per image
//     RandomHorizontalFlip -> RandomResizedCrop -> ColorJitter -> RandomGrayscale -> GaussianBlur(5 x 5)   on the image
//     the same flip and crop on meshgrid(linspace(-1,1,H), linspace(-1,1,W))                                 (coord_aug)
// (src/data.py:1082-1139, src/train_segmentation.py:602-610) with every image's own parameters, as two kernels for the whole batch:
//   k_augm_stats   only when some image has a contrast op: per block the resampled pixels of its tiles, the ops in front of the
//                  image's contrast op, the gray summed in fp64; one partial per block to the workspace (no atomics)
//   k_augm_apply   per output tile of 16 x 64: the resampled pixels of the tile (plus a 2-pixel halo where the image is blurred,
//                  reflected at the IMAGE border), the ops and the gray flag on every one of them, the three planes kept in LDS,
//                  the 5 x 5 blur from LDS, then img_aug and coord_aug written with 16-byte stores where the width allows
// No intermediate image reaches memory.  The per-image record (16 words) and the two coordinate ramps are device data made by the
// Python layer; the host entry has checked a host copy of the records, and axis_tap still holds every index inside the image.
// Arithmetic: the source position of a tap in fp64 from integers, exactly as aug_loss.crop_flip_coords forms it; everything behind it
// float32 in the order of torchvision's tensor transforms, one rounding per operation (contraction is off for this unit: the float32
// torch chain the tests hold this against rounds every product); the blur's weights, products and sum are fp64, rounded once per
// pixel; the contrast op's image mean is the fp64 sum of the float32 grays.
#include "dg_data_args.h"
#include "dg_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int TH = DG_AUGM_TH, TW = DG_AUGM_TW, HALO = 2, RH = TH + 2 * HALO, RW = TW + 2 * HALO, NT = DG_AUGM_THREADS;
static_assert(NT == TH * (TW / 4), "one thread per four neighbouring output pixels");
static_assert(RH <= 64 && RW <= 128 && NT >= 194, "the tap set-up gives rows the threads 0.., columns 64.., the two scalars 192 and 193");

struct Rec {
    int flip, top, left, bh, bw, ops[4], gray;
    float fac[4], sigma;
};

__device__ __forceinline__ Rec load_rec(const int32_t* __restrict__ recs, int b) {
    const int32_t* r = recs + (size_t)b * DG_AUGM_REC_WORDS;
    Rec R;
    R.flip = r[0]; R.top = r[1]; R.left = r[2]; R.bh = r[3]; R.bw = r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { R.ops[k] = r[5 + k]; R.fac[k] = __int_as_float(r[9 + k]); }
    R.gray = r[13];
    R.sigma = __int_as_float(r[14]);
    return R;
}

__device__ __forceinline__ int contrast_slot(const Rec& R) {
    int slot = -1;
#pragma unroll
    for (int k = 3; k >= 0; --k) if (R.ops[k] == DG_AUGM_CONTRAST) slot = k;
    return slot;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// position i of an axis of n outputs padded by reflection (no edge repeat); positions further out than the pad are held inside
__device__ __forceinline__ int reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return clampi(i, 0, n - 1);
}

// Output position o of an axis of n_out outputs that shows the crop [start, start + len) of an axis of dim pixels (bilinear,
// align_corners=False, taps held inside the crop): the two source pixels - mirrored where the image is flipped -, the fraction, and the
// coordinate ramp `lin` blended by them.  The position in fp64, the blend in float32: aug_loss.crop_flip_coords, operation for operation.
__device__ __forceinline__ void axis_tap(int o, int n_out, int start, int len, int dim, bool flip, const float* __restrict__ lin,
                                         int& s0, int& s1, float& f, float& coord) {
    const double scale = (double)len / (double)n_out;
    double src = ((double)o + 0.5) * scale - 0.5;
    const double hi = (double)(len - 1);
    src = src < 0.0 ? 0.0 : (src > hi ? hi : src);
    src += (double)start;
    int i0 = (int)floor(src);
    int i1 = min(i0 + 1, start + len - 1);
    f = (float)(src - (double)i0);
    i0 = clampi(i0, 0, dim - 1);                  // (a valid box never needs these two: device data is not trusted with an address)
    i1 = clampi(i1, 0, dim - 1);
    s0 = flip ? dim - 1 - i0 : i0;
    s1 = flip ? dim - 1 - i1 : i1;
    coord = lin[s0] * (1.0f - f) + lin[s1] * f;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
// torchvision's _blend: (ratio * img1 + (1 - ratio) * img2).clamp(0, 1)
__device__ __forceinline__ float blend(float x, float other, float f) { return clamp01(f * x + (1.0f - f) * other); }

// torchvision's adjust_hue on one pixel: _rgb2hsv, h = (h + f) mod 1, _hsv2rgb
__device__ __forceinline__ void hue_op(float& r, float& g, float& b, float f) {
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eq ? 1.0f : maxc);
    const float div = eq ? 1.0f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    const float hr = maxc == r ? bc - gc : 0.0f;
    const float hg = (maxc == g && maxc != r) ? 2.0f + rc - bc : 0.0f;
    const float hb = (maxc != g && maxc != r) ? 4.0f + gc - rc : 0.0f;
    float h = fmodf((hr + hg + hb) / 6.0f + 1.0f, 1.0f);
    h = fmodf(h + f, 1.0f);
    if (h < 0.0f) h += 1.0f;                       // torch's `%`: the result takes the divisor's sign
    const float h6 = h * 6.0f;
    const float fl = floorf(h6);
    const float fr = h6 - fl;
    const float v = maxc;
    const float p = clamp01(v * (1.0f - s));
    const float q = clamp01(v * (1.0f - s * fr));
    const float t = clamp01(v * (1.0f - s * (1.0f - fr)));
    int i = (int)fl % 6;
    if (i < 0) i += 6;
    r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
    g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
    b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// the image's ops of the slots [0, upto) on one pixel, in slot order; `mean`: the image mean of the gray for its contrast op
__device__ __forceinline__ void jitter(float& r, float& g, float& b, const Rec& R, int upto, float mean) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= upto) break;
        const int op = R.ops[k];
        const float f = op == DG_AUGM_BRIGHTNESS ? R.fac[0] : op == DG_AUGM_CONTRAST ? R.fac[1] : op == DG_AUGM_SATURATION ? R.fac[2] : R.fac[3];
        if (op == DG_AUGM_BRIGHTNESS) {
            r = blend(r, 0.0f, f); g = blend(g, 0.0f, f); b = blend(b, 0.0f, f);
        } else if (op == DG_AUGM_CONTRAST) {
            r = blend(r, mean, f); g = blend(g, mean, f); b = blend(b, mean, f);
        } else if (op == DG_AUGM_SATURATION) {
            const float l = gray_of(r, g, b);
            r = blend(r, l, f); g = blend(g, l, f); b = blend(b, l, f);
        } else if (op == DG_AUGM_HUE) {
            hue_op(r, g, b, f);
        }
    }
}

// the resampled pixel (three channels) of the taps (y0, y1, fy) x (x0, x1, fx), in the colour space the ops work in
__device__ __forceinline__ void resample(const DgAugmentArgs& A, const float* __restrict__ src, int y0, int y1, float fy, int x0, int x1,
                                         float fx, float* px) {
    const size_t plane = (size_t)A.H * A.W;
    const size_t r0 = (size_t)y0 * A.W, r1 = (size_t)y1 * A.W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = src + c * plane;
        const float top = p[r0 + x0] * (1.0f - fx) + p[r0 + x1] * fx;
        const float bot = p[r1 + x0] * (1.0f - fx) + p[r1 + x1] * fx;
        float v = top * (1.0f - fy) + bot * fy;
        if (!A.unit_space) v = v * A.stdv[c] + A.mean[c];
        px[c] = v;
    }
}

// the taps of the rows [oy0, oy0 + rh) and columns [ox0, ox0 + rw) of the output, reflected at its border: threads 0.. and 64..
struct TapSet {
    int y0[RH], y1[RH], x0[RW], x1[RW];
    float fy[RH], fx[RW], cy[RH], cx[RW];
};

__device__ __forceinline__ void make_taps(TapSet& T, const DgAugmentArgs& A, const Rec& R, int oy0, int ox0, int rh, int rw, int tid) {
    if (tid < rh) {
        axis_tap(reflect(oy0 + tid, A.h), A.h, R.top, R.bh, A.H, false, A.rows, T.y0[tid], T.y1[tid], T.fy[tid], T.cy[tid]);
    } else if (tid >= 64 && tid < 64 + rw) {
        const int k = tid - 64;
        axis_tap(reflect(ox0 + k, A.w), A.w, R.left, R.bw, A.W, R.flip != 0, A.cols, T.x0[k], T.x1[k], T.fx[k], T.cx[k]);
    }
}

}  // namespace

// grid (stat_blocks, B), block 256: block x of image b walks the tiles x, x + stat_blocks, ... and leaves one fp64 partial.
__global__ __launch_bounds__(DG_AUGM_THREADS) void k_augm_stats(DgAugmentArgs A) {
    __shared__ TapSet T;
    __shared__ double wave_part[NT / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Rec R = load_rec(A.recs, b);
    const int kc = contrast_slot(R);
    if (kc < 0) return;                             // (the whole block: the record is uniform)
    const float* src = A.img + (size_t)b * 3 * A.H * A.W;
    double acc = 0.0;
    const int n_tiles = A.tiles_x * A.tiles_y;
    for (int t = blockIdx.x; t < n_tiles; t += A.stat_blocks) {
        const int oy0 = (t / A.tiles_x) * TH, ox0 = (t % A.tiles_x) * TW;
        __syncthreads();                            // the last tile's taps have been read
        make_taps(T, A, R, oy0, ox0, TH, TW, tid);
        __syncthreads();
        for (int idx = tid; idx < TH * TW; idx += NT) {
            const int ly = idx / TW, lx = idx - ly * TW;
            if (oy0 + ly >= A.h || ox0 + lx >= A.w) continue;
            float px[3];
            resample(A, src, T.y0[ly], T.y1[ly], T.fy[ly], T.x0[lx], T.x1[lx], T.fx[lx], px);
            jitter(px[0], px[1], px[2], R, kc, 0.0f);
            acc += (double)gray_of(px[0], px[1], px[2]);
        }
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < NT / 64; ++k) s += wave_part[k];
        A.partials[(size_t)b * A.stat_blocks + blockIdx.x] = s;
    }
}

// grid (tiles_x, tiles_y, B), block 256, 18.2 KB of LDS.
__global__ __launch_bounds__(DG_AUGM_THREADS) void k_augm_apply(DgAugmentArgs A) {
    __shared__ __align__(16) float plane[3][RH * RW];
    __shared__ TapSet T;
    __shared__ double wtap[5];
    __shared__ float s_mean;
    const int b = blockIdx.z, tid = threadIdx.x;
    const Rec R = load_rec(A.recs, b);
    const bool blur = R.sigma > 0.0f;
    const int pad = blur ? HALO : 0;
    const int rh = TH + 2 * pad, rw = TW + 2 * pad;
    const int ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;

    make_taps(T, A, R, ty0 - pad, tx0 - pad, rh, rw, tid);
    if (tid == 192) {
        float m = 0.0f;
        if (contrast_slot(R) >= 0) {                // the image's partials, in block order
            double s = 0.0;
            for (int k = 0; k < A.stat_blocks; ++k) s += A.partials[(size_t)b * A.stat_blocks + k];
            m = (float)(s / ((double)A.h * (double)A.w));
        }
        s_mean = m;
    } else if (tid == 193 && blur) {                // exp(-0.5 (x / sigma)^2) on x = -2..2, normalised
        const double sg = (double)R.sigma;
        const double e1 = exp(-0.5 * (1.0 / sg) * (1.0 / sg)), e2 = exp(-0.5 * (2.0 / sg) * (2.0 / sg));
        const double sum = 1.0 + 2.0 * e1 + 2.0 * e2;
        wtap[0] = wtap[4] = e2 / sum;
        wtap[1] = wtap[3] = e1 / sum;
        wtap[2] = 1.0 / sum;
    }
    __syncthreads();

    const float* src = A.img + (size_t)b * 3 * A.H * A.W;
    const float mean = s_mean;
    for (int idx = tid; idx < rh * rw; idx += NT) {
        const int ry = idx / rw, rx = idx - ry * rw;
        float px[3];
        resample(A, src, T.y0[ry], T.y1[ry], T.fy[ry], T.x0[rx], T.x1[rx], T.fx[rx], px);
        jitter(px[0], px[1], px[2], R, 4, mean);
        if (R.gray) px[0] = px[1] = px[2] = gray_of(px[0], px[1], px[2]);
        plane[0][ry * RW + rx] = px[0];
        plane[1][ry * RW + rx] = px[1];
        plane[2][ry * RW + rx] = px[2];
    }
    __syncthreads();

    const int ly = tid / (TW / 4), lx = (tid % (TW / 4)) * 4;
    const int oy = ty0 + ly, ox = tx0 + lx;
    if (oy >= A.h || ox >= A.w) return;
    float out[3][4];
    if (blur) {
        // the 25 products and their sum in fp64 from the five fp64 weights (a row's five taps, then the five rows), rounded once: the
        // blur adds half a float32 spacing to what it is handed, whatever sigma is
        double wt[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) wt[k] = wtap[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) {
                const float4* row = reinterpret_cast<const float4*>(&plane[c][(ly + ky) * RW + lx]);      // 16-byte aligned: RW and lx are multiples of 4
                const float4 a = row[0], d = row[1];
                const float v[8] = {a.x, a.y, a.z, a.w, d.x, d.y, d.z, d.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    double r = 0.0;
#pragma unroll
                    for (int kx = 0; kx < 5; ++kx) r = fma(wt[kx], (double)v[j + kx], r);
                    acc[j] = fma(wt[ky], r, acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) out[c][j] = (float)acc[j];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 a = *reinterpret_cast<const float4*>(&plane[c][ly * RW + lx]);
            out[c][0] = a.x; out[c][1] = a.y; out[c][2] = a.z; out[c][3] = a.w;
        }
    }
    if (!A.unit_space) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) out[c][j] = (out[c][j] - A.mean[c]) / A.stdv[c];
    }

    const size_t oplane = (size_t)A.h * A.w, opix = (size_t)oy * A.w + ox;
    float* dst = A.img_aug + (size_t)b * 3 * oplane + opix;
    float* dstc = A.coord_aug + ((size_t)b * oplane + opix) * 2;
    const float cy = T.cy[ly + pad];
    const float cx[4] = {T.cx[lx + pad], T.cx[lx + pad + 1], T.cx[lx + pad + 2], T.cx[lx + pad + 3]};
    if (A.vec_stores) {                             // w % 4 == 0 and both bases 16-byte aligned: the four pixels exist and every address is aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(dst + c * oplane) = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
        float4* c4 = reinterpret_cast<float4*>(dstc);
        c4[0] = make_float4(cy, cx[0], cy, cx[1]);
        c4[1] = make_float4(cy, cx[2], cy, cx[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (ox + j >= A.w) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c * oplane + j] = out[c][j];
            dstc[2 * j] = cy;
            dstc[2 * j + 1] = cx[j];
        }
    }
}

hipError_t dg_launch_augment(const DgAugmentArgs& A, bool stats, hipStream_t s) {
    if (stats) {
        hipLaunchKernelGGL(k_augm_stats, dim3(A.stat_blocks, A.B), dim3(DG_AUGM_THREADS), 0, s, A);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_augm_apply, dim3(A.tiles_x, A.tiles_y, A.B), dim3(DG_AUGM_THREADS), 0, s, A);
    return hipGetLastError();
}
