// The reconstruction loss term of the training step (cfg.rec_weight; src/train_segmentation.py:391-398):
//     rec_feats = decoder(code)                                  (nn.Conv2d(dim, n_feats, (1,1)), src/train_segmentation.py:115)
//     loss      = -mean over (b,i,j) of <norm(rec_feats), norm(feats)>     (src/modules.py:789-790: F.normalize(dim=1, eps=1e-10))
// Per position p (N = B h w of them), y = W c_p + bias (C values from the D of code), f = feats at p:
//     ny = max(|y|, eps), nf = max(|f|, eps), s = <y, f> / (ny nf), loss = -(1/N) sum s
//     dy = a f + b y,  a = -(G/N) / (ny nf),  b = (G/N) s / ny^2 where |y| > eps, else 0 (clamp_min passes no gradient below its bound)
//     d code_p = W^T dy,  d W = sum_p dy c_p^T,  d bias = sum_p dy
//     d f = a y + b' f,  b' = (G/N) s / nf^2 where |f| > eps, else 0 - dy's mirror image, opt-in (dg_rec_feats_backward): feats is the
//     frozen backbone's output except under the depth-guided featurizer, whose trained depth modules produced it
// Neither y, the normalised maps nor dy exist in global memory: every kernel re-forms y for the channels it is at.  The three
// products run on the fp32 MFMA (v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulation, as dg_knn.hip) from LDS: a block holds
// a tile of 64 positions of code ([d][p], rows of 65 words, zero rows up to the next multiple of 32), one chunk of RC_CHUNK = 64
// decoder rows of W ([c][d], zero-padded to a multiple of 8 columns) staged with coalesced vector loads - W is streamed chunk by
// chunk, any C - and a chunk of dy ([c][p], rows of 65 words).  The MFMA's operands (dg_knn.hip has them measured): lane (r, h) =
// (lane & 31, lane >> 5) gives A[row r][k = h] and B[column r][k = h]; accumulator element i of the lane is row
// (i & 3) + 8 (i >> 2) + 4 h, column r.  Five kernels, two forward and three backward:
//   k_rec_forward   one block per tile; wave w takes the positions 32 (w & 1) .. + 31 and the channels 32 (w >> 1) .. + 31 of every
//                   chunk: y = rows of W x the code tile, the sum over d as four interleaved accumulator tiles (d mod 4) added
//                   pairwise; a lane then holds 16 channels of one position: |y|^2, |f|^2, <y,f> over the channels in fp64, the
//                   two half waves and the two channel halves combined in one order; |y|, |f|, s to the workspace, the tile's sum
//                   of -s as one double
//   k_loss_reduce   the tiles' sums -> the loss (fp64, fixed order; dg_loss_reduce.hip)
//   k_rec_bwd_code  per tile again: y and dy of a chunk -> LDS, then W^T dy of the chunk is added to the wave's accumulator tiles
//                   (32 rows of d code x 32 positions each) which live through all chunks; every element of d code written.
//                   <true>: the wave also stores d f of the 32 channels x 32 positions whose y, f and factors it holds, from
//                   its registers in the accumulator layout (an accumulator row is 32 consecutive positions of one channel: 128
//                   contiguous bytes per half wave), every element of d feats once; without grad_code the W^T dy product is skipped
//   k_rec_bwd_w     grid (channel chunk, split): the chunk of W staged once, the block walks the tiles split, split + S, ...: dy of
//                   its 64 channels into LDS, then dy c^T over the tile's 64 positions into accumulator tiles (32 channels x 32 rows
//                   of d W) that live through all its tiles; one partial of d W / d bias per (split, chunk)
//   k_rec_combine   the S partials -> d W, d bias (fp64, fixed order); every element written
// y, dy and the three products are fp32; the forward's three sums over the channels run in fp64 (with fp32 sums a 1024-channel
// decoder measured 8 x the float32 torch chain's loss error); no atomics; every result is a function of the inputs alone, bit for bit.
// Dropout2d keep flags (ops.DeferredDropout): f = feats * (keep[b,c] ? scale : 0), the bits of the materialised tensor; d feats is
// then the gradient of the un-dropped maps the pointer names: d f times (keep[b,c] ? scale : 0), a dropped channel an exact 0.
#include "dg_loss_args.h"
#include "dg_device.h"

#define RC_THREADS 256
#define RC_TP DG_REC_TP                 // positions per tile
#define RC_CHUNK DG_REC_CHUNK           // decoder rows staged at once
#define RC_LS 65                        // row stride of the code and dy tiles: conflict-free along a row and across rows

static_assert(RC_TP == 64 && RC_CHUNK == 64 && RC_THREADS == 256, "four waves: two position halves x two channel halves");

// The block's LDS (dg_rec_lds(D) bytes): dy chunk [64][65] (the forward keeps its sums there), W chunk [64][ws], code tile [dr][65].
struct RecLds { float* dyl; float* wl; float* tile; int dp, ws, dr; };
__device__ __forceinline__ RecLds rec_lds(float* base, int D) {
    RecLds L;
    L.dp = (D + 7) & ~7; L.ws = L.dp + 4; L.dr = (D + 31) & ~31;
    L.dyl = base; L.wl = base + RC_CHUNK * RC_LS; L.tile = L.wl + RC_CHUNK * L.ws;
    return L;
}
__device__ __forceinline__ int rec_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }     // accumulator element -> tile row

struct RecTile { int b, p0; };
__device__ __forceinline__ RecTile rec_tile(int tile, int tpi) {
    RecTile t;
    t.b = tile / tpi; t.p0 = (tile - t.b * tpi) * RC_TP;
    return t;
}

// code[b, :, p0 .. p0 + 63] -> tile[d * RC_LS + l]; zero past the image's last position and in the rows D .. dr - 1
__device__ __forceinline__ void rec_load_code(const float* __restrict__ code, const RecLds& L, int b, int p0, int D, int P) {
    const float* src = code + (size_t)b * D * P;
    // (dr is a multiple of 32: eight independent loads a thread and step, so their latencies overlap)
    for (int base = threadIdx.x; base < L.dr * RC_TP; base += 8 * RC_THREADS) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * RC_THREADS, d = i >> 6, p = p0 + (i & 63);
            v[u] = (d < D && p < P) ? src[(size_t)d * P + p] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * RC_THREADS;
            L.tile[(i >> 6) * RC_LS + (i & 63)] = v[u];
        }
    }
}

// W[cb .. cb + 63, :] -> wl[row * ws + d]; zero rows past C, zero columns D .. dp - 1.  A wave takes 16 rows, its lanes run along d.
__device__ __forceinline__ void rec_load_w(const float* __restrict__ W, const RecLds& L, int cb, int C, int D, int wave, int lane) {
    const int row0 = wave * (RC_CHUNK / 4);
    for (int d = lane; d < L.dp; d += 64) {                     // (the 16 rows' loads are independent: their latencies overlap)
        float v[RC_CHUNK / 4];
#pragma unroll
        for (int k = 0; k < RC_CHUNK / 4; ++k) {
            const int c = cb + row0 + k;
            v[k] = (c < C && d < D) ? W[(size_t)c * D + d] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < RC_CHUNK / 4; ++k) L.wl[(row0 + k) * L.ws + d] = v[k];
    }
}

// y without the bias: rows crow .. crow + 31 of the staged chunk x the positions 32 pb .. + 31 of the tile.  Half wave h takes
// d = 8 j + 4 h .. + 3 of every step of 8 (a dot product does not care which two d share an MFMA); MFMA q of a step adds to
// accumulator tile q: four interleaved chains over d, a quarter of the chain length each, added pairwise - with ONE chain of FMAs
// the training widths (D = 70, C = 384, 128 positions) measured 3 float32 spacings of loss error, the float32 torch chain 1.
__device__ __forceinline__ f32x16 rec_y(const RecLds& L, int crow, int pb, int r, int h) {
    f32x16 a0 = {}, a1 = {}, a2 = {}, a3 = {};
    const float* wa = L.wl + (crow + r) * L.ws + 4 * h;
    const float* tb = L.tile + (4 * h) * RC_LS + pb * 32 + r;
    for (int d0 = 0; d0 < L.dp; d0 += 8) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(wa + d0);
        const float* t = tb + d0 * RC_LS;
        const float b0 = t[0], b1 = t[RC_LS], b2 = t[2 * RC_LS], b3 = t[3 * RC_LS];
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1, a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b2, a2, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b3, a3, 0, 0, 0);
    }
    return (a0 + a1) + (a2 + a3);
}

// feats[b, c, p] with its Dropout2d flag applied; 0 for a channel past C or a position past P
__device__ __forceinline__ float rec_f(const DgRecArgs& A, int b, int c, int p) {
    if (c >= A.C || p >= A.P) return 0.f;
    const float m = A.keep ? (A.keep[(size_t)b * A.C + c] != 0.f ? A.scale : 0.f) : 1.f;
    return A.feats[((size_t)b * A.C + c) * A.P + p] * m;
}

// the lane's 16 channels (accumulator rows) of f for the 32 channels at c0: issued before the staging loads so that all are in flight together
__device__ __forceinline__ void rec_f16(const DgRecArgs& A, int b, int c0, int h, int p, float (&f)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = rec_f(A, b, c0 + rec_row(i, h), p);
}

// the two factors of dy = a f + b y at one position; both 0 past the image's last position
__device__ __forceinline__ void rec_factors(const DgRecArgs& A, int b, int p, float& fa, float& fb) {
    fa = 0.f; fb = 0.f;
    if (p < A.P) {
        const size_t r = (size_t)b * A.P + p;
        const float ny = A.ny[r], nf = A.nf[r], s = A.s[r];
        const float gn = (float)((double)A.grad_out[0] * A.inv_n);
        const float nyc = fmaxf(ny, DG_EPS_NORM), nfc = fmaxf(nf, DG_EPS_NORM);
        fa = -gn / (nyc * nfc);
        fb = ny > DG_EPS_NORM ? gn * s / (nyc * nyc) : 0.f;
    }
}

// b' of d f = a y + b' f at one position; 0 past the image's last position and where |f| <= eps (the rule b follows for |y|)
__device__ __forceinline__ float rec_factor_f(const DgRecArgs& A, int b, int p) {
    if (p >= A.P) return 0.f;
    const size_t r = (size_t)b * A.P + p;
    const float nf = A.nf[r], s = A.s[r];
    const float gn = (float)((double)A.grad_out[0] * A.inv_n);
    const float nfc = fmaxf(nf, DG_EPS_NORM);
    return nf > DG_EPS_NORM ? gn * s / (nfc * nfc) : 0.f;
}

// grid B * tiles_per_img, block 256, dynamic LDS dg_rec_lds(D).
__global__ __launch_bounds__(RC_THREADS) void k_rec_forward(const DgRecArgs A) {
    extern __shared__ float4 rec_smem[];
    const RecLds L = rec_lds(reinterpret_cast<float*>(rec_smem), A.D);
    double* red = reinterpret_cast<double*>(L.dyl);             // [3][2 channel halves][64 positions]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5, pb = wave & 1, ch = wave >> 1;
    const RecTile t = rec_tile(blockIdx.x, A.tiles_per_img);
    const int p = t.p0 + pb * 32 + r;
    rec_load_code(A.code, L, t.b, t.p0, A.D, A.P);
    double yy = 0.0, ff = 0.0, yf = 0.0;
    for (int cb = 0; cb < A.C; cb += RC_CHUNK) {
        const int c0 = cb + ch * 32;
        float f[16];
        rec_f16(A, t.b, c0, h, p, f);
        __syncthreads();                                        // the last chunk's readers are done
        rec_load_w(A.weight, L, cb, A.C, A.D, wave, lane);
        __syncthreads();
        if (c0 >= A.C) continue;                                // (wave-uniform; both barriers are above)
        const f32x16 y = rec_y(L, ch * 32, pb, r, h);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = c0 + rec_row(i, h);
            if (c < A.C) {
                const double yd = (double)(y[i] + A.bias[c]), fd = (double)f[i];
                yy = fma(yd, yd, yy); ff = fma(fd, fd, ff); yf = fma(yd, fd, yf);
            }
        }
    }
    yy += __shfl_xor(yy, 32, 64); ff += __shfl_xor(ff, 32, 64); yf += __shfl_xor(yf, 32, 64);
    __syncthreads();                                            // (the dy region held nothing, but the W loads are behind us)
    if (h == 0) {
        red[(0 * 2 + ch) * 64 + pb * 32 + r] = yy;
        red[(1 * 2 + ch) * 64 + pb * 32 + r] = ff;
        red[(2 * 2 + ch) * 64 + pb * 32 + r] = yf;
    }
    __syncthreads();
    if (wave != 0) return;
    double neg = 0.0;
    const int q = t.p0 + lane;
    if (q < A.P) {
        const double syy = red[0 * 64 + lane] + red[1 * 64 + lane], sff = red[2 * 64 + lane] + red[3 * 64 + lane],
                     syf = red[4 * 64 + lane] + red[5 * 64 + lane];
        const double ny = sqrt(syy), nf = sqrt(sff);
        const double s = syf / fmax(ny, (double)DG_EPS_NORM) / fmax(nf, (double)DG_EPS_NORM);
        const size_t row = (size_t)t.b * A.P + q;
        A.ny[row] = (float)ny; A.nf[row] = (float)nf; A.s[row] = (float)s;
        neg = -s;
    }
    neg = wave_sum(neg);
    if (lane == 0) A.part[blockIdx.x] = neg;
}

// dy of the wave's 32 channels x 32 positions of the staged chunk -> dyl[row * RC_LS + position]; 0 for a channel past C.
// FEATS: d f = (a y + b' f) (keep ? scale : 0) of the same elements -> grad_feats (b: the image, p: the lane's position, fbf: b');
// channels past C and positions past P are not stored.
template <bool FEATS>
__device__ __forceinline__ void rec_dy(const DgRecArgs& A, const RecLds& L, const float (&f)[16], int cb, int ch, int pb, int r, int h,
                                       float fa, float fb, float fbf = 0.f, int b = 0, int p = 0) {
    const int c0 = cb + ch * 32;
    if (c0 < A.C) {
        const f32x16 y = rec_y(L, ch * 32, pb, r, h);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = c0 + rec_row(i, h);
            L.dyl[(ch * 32 + rec_row(i, h)) * RC_LS + pb * 32 + r] = c < A.C ? fmaf(fa, f[i], fb * (y[i] + A.bias[c])) : 0.f;
            if constexpr (FEATS) {
                if (c < A.C && p < A.P) {
                    const float m = A.keep ? (A.keep[(size_t)b * A.C + c] != 0.f ? A.scale : 0.f) : 1.f;
                    const float df = fmaf(fa, y[i] + A.bias[c], fbf * f[i]);
                    A.grad_feats[((size_t)b * A.C + c) * A.P + p] = m != 0.f ? df * m : 0.f;
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) L.dyl[(ch * 32 + rec_row(i, h)) * RC_LS + pb * 32 + r] = 0.f;
    }
}

// d code (B,D,h,w), every element written.  grid B * tiles_per_img, block 256, dynamic LDS dg_rec_lds(D).
// FEATS: d feats (B,C,h,w) as well, every element written; grad_code may then be null (no W^T dy product, d code not stored).
template <bool FEATS>
__global__ __launch_bounds__(RC_THREADS) void k_rec_bwd_code(const DgRecArgs A) {
    extern __shared__ float4 rec_smem[];
    const RecLds L = rec_lds(reinterpret_cast<float*>(rec_smem), A.D);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5, pb = wave & 1, ch = wave >> 1;
    const RecTile t = rec_tile(blockIdx.x, A.tiles_per_img);
    const int p = t.p0 + pb * 32 + r;
    rec_load_code(A.code, L, t.b, t.p0, A.D, A.P);
    float fa, fb;
    rec_factors(A, t.b, p, fa, fb);
    float fbf = 0.f;
    if constexpr (FEATS) fbf = rec_factor_f(A, t.b, p);
    const bool want_code = !FEATS || A.grad_code != nullptr;   // (block-uniform; a constant without FEATS)
    // the wave's tiles of d code: rows 32 m .. + 31 for m = ch and ch + 2, its 32 positions
    f32x16 acc[2] = {{}, {}};
    for (int cb = 0; cb < A.C; cb += RC_CHUNK) {
        float f[16];
        rec_f16(A, t.b, cb + ch * 32, h, p, f);
        __syncthreads();
        rec_load_w(A.weight, L, cb, A.C, A.D, wave, lane);
        __syncthreads();
        rec_dy<FEATS>(A, L, f, cb, ch, pb, r, h, fa, fb, fbf, t.b, p);
        __syncthreads();
        if (!want_code) continue;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = ch + 2 * u;
            if (m * 32 >= A.D) continue;
            const int col = m * 32 + r < L.dp ? m * 32 + r : L.dp - 1;      // (a row of d code past D repeats one and is not written)
            const float* wa = L.wl + h * L.ws + col;
            const float* db = L.dyl + h * RC_LS + pb * 32 + r;
#pragma unroll 8
            for (int k = 0; k < RC_CHUNK; k += 2)
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[k * L.ws], db[k * RC_LS], acc[u], 0, 0, 0);
        }
    }
    if (want_code && p < A.P) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int d = (ch + 2 * u) * 32 + rec_row(i, h);
                if (d < A.D) A.grad_code[((size_t)t.b * A.D + d) * A.P + p] = acc[u][i];
            }
    }
}

// One partial of d W and d bias per (split, chunk): wpart[(split * C + c) * D + d], bpart[split * C + c].
// grid (chunks of RC_CHUNK channels, splits), block 256, dynamic LDS dg_rec_lds(D).
__global__ __launch_bounds__(RC_THREADS) void k_rec_bwd_w(const DgRecArgs A) {
    extern __shared__ float4 rec_smem[];
    const RecLds L = rec_lds(reinterpret_cast<float*>(rec_smem), A.D);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5, pb = wave & 1, ch = wave >> 1;
    const int cb = blockIdx.x * RC_CHUNK, split = blockIdx.y, tiles = A.B * A.tiles_per_img;
    rec_load_w(A.weight, L, cb, A.C, A.D, wave, lane);
    // the wave's tiles of d W: channels 32 cg .. + 31 of the chunk (cg = wave & 1) x rows 32 m .. + 31 for m = wave >> 1 and + 2
    const int cg = wave & 1;
    f32x16 acc[2] = {{}, {}};
    // d bias of channel cb + (thread >> 2): each of a row's four threads sums 16 positions of dy in fp64, the four are added as
    // (0 + 1) + (2 + 3)
    double db = 0.0;
    for (int it = split; it < tiles; it += A.splits) {
        const RecTile t = rec_tile(it, A.tiles_per_img);
        const int p = t.p0 + pb * 32 + r;
        float f[16], fa, fb;
        rec_f16(A, t.b, cb + ch * 32, h, p, f);
        rec_factors(A, t.b, p, fa, fb);
        __syncthreads();                                        // the last tile's readers are done with both tiles
        rec_load_code(A.code, L, t.b, t.p0, A.D, A.P);
        __syncthreads();
        rec_dy<false>(A, L, f, cb, ch, pb, r, h, fa, fb);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = (wave >> 1) + 2 * u;
            if (m * 32 >= A.D) continue;
            const float* da = L.dyl + (cg * 32 + r) * RC_LS + h;
            const float* cbp = L.tile + (m * 32 + r) * RC_LS + h;
#pragma unroll 8
            for (int k = 0; k < RC_TP; k += 2) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(da[k], cbp[k], acc[u], 0, 0, 0);
        }
        {
            const float* row = L.dyl + (threadIdx.x >> 2) * RC_LS + (threadIdx.x & 3) * 16;
            double sdb = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) sdb += (double)row[k];
            sdb += __shfl_xor(sdb, 1, 64);
            sdb += __shfl_xor(sdb, 2, 64);
            db += sdb;
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int d = ((wave >> 1) + 2 * u) * 32 + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = cb + cg * 32 + rec_row(i, h);
            if (c < A.C && d < A.D) A.wpart[((size_t)split * A.C + c) * A.D + d] = acc[u][i];
        }
    }
    if ((threadIdx.x & 3) == 0 && cb + (int)(threadIdx.x >> 2) < A.C) A.bpart[(size_t)split * A.C + cb + (threadIdx.x >> 2)] = (float)db;
}

// d W (C,D) and d bias (C), every element written: the splits' partials summed in fp64 in split order.
// grid ceil((C D + C) / 256), block 256.
__global__ __launch_bounds__(256) void k_rec_combine(const DgRecArgs A) {
    const size_t nw = (size_t)A.C * A.D, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw + A.C) return;
    const bool is_w = i < nw;
    const float* src = is_w ? A.wpart + i : A.bpart + (i - nw);
    const size_t stride = is_w ? nw : (size_t)A.C;
    double s = 0.0;
    for (int k = 0; k < A.splits; ++k) s += (double)src[(size_t)k * stride];
    (is_w ? A.grad_weight[i] : A.grad_bias[i - nw]) = (float)s;
}

static hipError_t rec_smem_limit(const void* kern, int lds) {
    return lds > 64 * 1024 ? dg_set_max_smem(kern, lds) : hipSuccess;
}

hipError_t dg_launch_rec_forward(const DgRecArgs& A, hipStream_t s) {
    const int tiles = A.B * A.tiles_per_img, lds = (int)dg_rec_lds(A.D);
    const hipError_t e = dg_launch_if(lds > 64 * 1024, k_rec_forward, dim3(tiles), dim3(RC_THREADS), lds, s, A);
    if (e != hipSuccess) return e;
    return dg_launch_loss_reduce(A.part, tiles, A.inv_n, A.loss, s);
}

// FEATS: k_rec_bwd_code<true> in place of <false>; params: the d W / d bias launches behind it
template <bool FEATS>
static hipError_t rec_backward(const DgRecArgs& A, bool params, hipStream_t s) {
    const int tiles = A.B * A.tiles_per_img, chunks = (A.C + RC_CHUNK - 1) / RC_CHUNK, lds = (int)dg_rec_lds(A.D);
    hipError_t e = rec_smem_limit(reinterpret_cast<const void*>(k_rec_bwd_code<FEATS>), lds);
    if (e != hipSuccess) return e;
    e = rec_smem_limit(reinterpret_cast<const void*>(k_rec_bwd_w), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rec_bwd_code<FEATS>, dim3(tiles), dim3(RC_THREADS), lds, s, A);
    e = hipGetLastError();
    if (e != hipSuccess || !params) return e;
    hipLaunchKernelGGL(k_rec_bwd_w, dim3(chunks, A.splits), dim3(RC_THREADS), lds, s, A);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t outs = (size_t)A.C * A.D + A.C;
    hipLaunchKernelGGL(k_rec_combine, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, A);
    return hipGetLastError();
}

hipError_t dg_launch_rec_backward(const DgRecArgs& A, hipStream_t s) { return rec_backward<false>(A, true, s); }

hipError_t dg_launch_rec_backward_feats(const DgRecArgs& A, hipStream_t s) {
    if (!A.grad_feats) return hipErrorInvalidValue;
    return rec_backward<true>(A, A.grad_code != nullptr, s);
}
