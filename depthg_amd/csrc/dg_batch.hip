// Batch preparation (depthg_amd/data.py): the loader transform of the training data path for a whole batch - the samples and their
// kNN positives - in ONE launch.  The reference's get_transform (src/utils.py:164-182) is
//     Resize(res, NEAREST) -> cropper -> ToTensor -> Normalize      on the image
//     Resize(res, NEAREST) -> cropper -> ToTargetTensor             on the label and the depth map
// per sample on the CPU: a gather per output pixel, then two float32 operations.  Here the decoded uint8 planes of all samples lie in
// one packed device buffer, every source at its own size; the resize and the crop are composed on the host into two index tables
// per sample (xs[W]: the source column of every output column, ys[H]: the source row of every output row), and a record per output
// plane group says where the source lies and what to write:
//     image        (N,3,H,W) float32  (byte / 255 - mean[c]) / std[c]      ToTensor's division, then Normalize's sub and div
//     label        (N,H,W)   int64    byte + label_offset                    and the mask: bool (label == -1) or float32 (label > 0)
//     depth        (N,H,W)   float32  the byte value; the plane variant and the constant label read no source
// Output-stationary: grid (tiles of 16 rows x 64 columns, records), one lane per four neighbouring output columns of a row.  The
// block's 16 row indices and 64 column indices are read once into LDS; every float32 and int64 store is a whole 16-byte vector (the
// byte mask's four columns are one 4-byte word).  W is a multiple of 4 and every output 16-byte aligned: the host entry refuses
// anything else, so no lane has a partial vector.  No atomics, no intermediate image; each output element is written by exactly one
// lane of one record (the host entry checks that the records cover every sample once), so two calls give the same bytes.
// Arithmetic: float32 with IEEE division and no contraction - the bits of torch's CPU chain.
// The records and tables are device data: the host entry has checked a host copy, and the kernel still holds every index inside
// its plane.
#include "dg_aux_args.h"
#include "dg_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int TH = DG_BATCH_TH, TW = DG_BATCH_TW, NT = DG_BATCH_THREADS;
static_assert(NT == TH * (TW / 4), "one thread per four neighbouring output pixels");
static_assert(NT >= TW + TH, "the tables of a tile are read by the threads 0 .. TW + TH - 1");

}  // namespace

// grid (tiles_x * tiles_y, n_records), block 256, 320 bytes of LDS.
__global__ __launch_bounds__(DG_BATCH_THREADS) void k_batch_prep(DgBatchArgs A) {
    __shared__ int s_x[TW], s_y[TH];
    const int tid = threadIdx.x;
    const int32_t* r = A.recs + (size_t)blockIdx.y * DG_BATCH_REC_WORDS;
    const int kind = r[0], n = r[1];
    const size_t src_off = (size_t)(uint32_t)r[2] | ((size_t)(uint32_t)r[3] << 32);
    const int sw = r[4], sh = r[5], label_offset = r[6], mask_rule = r[7];
    const int ty0 = (blockIdx.x / A.tiles_x) * TH, tx0 = (blockIdx.x % A.tiles_x) * TW;
    const bool reads = kind == DG_BATCH_IMAGE || kind == DG_BATCH_LABEL || kind == DG_BATCH_DEPTH;

    if (reads) {                                    // (the record is uniform over the block: so is the barrier)
        const int32_t* xs = A.tables + (size_t)n * (A.W + A.H);
        const int32_t* ys = xs + A.W;
        if (tid < TW) {
            s_x[tid] = tx0 + tid < A.W ? dg_hold(xs[tx0 + tid], sw) : 0;
        } else if (tid < TW + TH) {
            const int k = tid - TW;
            s_y[k] = ty0 + k < A.H ? dg_hold(ys[ty0 + k], sh) : 0;
        }
        __syncthreads();
    }

    const int ly = tid / (TW / 4), lx = (tid % (TW / 4)) * 4;
    const int oy = ty0 + ly, ox = tx0 + lx;
    if (oy >= A.H || ox >= A.W) return;             // W % 4 == 0: a lane has its four columns or none
    const size_t oplane = (size_t)A.H * A.W, opix = (size_t)oy * A.W + ox;
    const uint8_t* src = A.packed + src_off;

    if (kind == DG_BATCH_IMAGE) {
        const uint8_t* row = src + (size_t)s_y[ly] * sw * 3;
        float v[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint8_t* px = row + (size_t)s_x[lx + j] * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = dg_normalized_byte(px[c], A.mean[c], A.stdv[c]);
        }
        float* dst = A.img + (size_t)n * 3 * oplane + opix;
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(dst + c * oplane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else if (kind == DG_BATCH_LABEL || kind == DG_BATCH_LABEL_FILL) {
        long long lab[4];
        if (kind == DG_BATCH_LABEL) {
            const uint8_t* row = src + (size_t)s_y[ly] * sw;
#pragma unroll
            for (int j = 0; j < 4; ++j) lab[j] = (long long)row[s_x[lx + j]] + label_offset;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) lab[j] = label_offset;
        }
        longlong2* dst = reinterpret_cast<longlong2*>(A.label + (size_t)n * oplane + opix);
        dst[0] = make_longlong2(lab[0], lab[1]);
        dst[1] = make_longlong2(lab[2], lab[3]);
        if (mask_rule == DG_BATCH_MASK_FLOAT_POSITIVE) {
            float* m = static_cast<float*>(A.mask) + (size_t)n * oplane + opix;
            *reinterpret_cast<float4*>(m) = make_float4(lab[0] > 0 ? 1.0f : 0.0f, lab[1] > 0 ? 1.0f : 0.0f, lab[2] > 0 ? 1.0f : 0.0f,
                                                        lab[3] > 0 ? 1.0f : 0.0f);
        } else {                                    // DG_BATCH_MASK_BOOL_IGNORED: torch.bool is one byte, 0 / 1
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) word |= (lab[j] == -1 ? 1u : 0u) << (8 * j);
            uint8_t* m = static_cast<uint8_t*>(A.mask) + (size_t)n * oplane + opix;
            *reinterpret_cast<uint32_t*>(m) = word;
        }
    } else if (kind == DG_BATCH_DEPTH || kind == DG_BATCH_DEPTH_PLANE) {
        float d[4] = {255.0f, 255.0f, 255.0f, 255.0f};
        if (kind == DG_BATCH_DEPTH) {
            const uint8_t* row = src + (size_t)s_y[ly] * sw;
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = (float)row[s_x[lx + j]];
        }
        *reinterpret_cast<float4*>(A.depth + (size_t)n * oplane + opix) = make_float4(d[0], d[1], d[2], d[3]);
    }
}

hipError_t dg_launch_batch_prep(const DgBatchArgs& A, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_prep, dim3(A.tiles_x * A.tiles_y, A.n_records), dim3(DG_BATCH_THREADS), 0, s, A);
    return hipGetLastError();
}
