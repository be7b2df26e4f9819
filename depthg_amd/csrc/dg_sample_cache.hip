// Device-resident sample cache (depthg_amd/sample_cache.py).  With a deterministic loader crop the resized and cropped bytes of every
// image, label and depth map (src/utils.py:164-182) are the same in every epoch, and so is everything the reference's datasets form
// from them (src/data.py:894-902, :126-128).  The cache keeps those bytes on the card as uint8 (n_images, planes, H, W) at the
// loader's OUTPUT size - planes R, G, B, then the label if the dataset has labels, then the depth if it is wanted - and a batch and
// its kNN positives come back in the step's dtypes from one launch, with no file, no decoder, no pinned buffer and no upload:
//   k_sc_put     rows idx[0..n) of the cache = the bytes k_batch_prep's nearest resize and crop select from the packed source planes
//                (its records, its tables, its 16 x 64 tiles with the tile's tables read once into LDS and held inside the plane),
//                without its arithmetic.  Image HWC becomes three planes; a DG_BATCH_DEPTH_PLANE record stores the byte 255 (float(255)
//                is what k_batch_prep writes for that kind); a DG_BATCH_LABEL_FILL record writes nothing (such a cache has no label
//                plane).  A lane owns four neighbouring columns of a row and stores them as one 32-bit word per plane.
//   k_sc_gather  rows 0..n-1 from idx_a, rows n..2n-1 from idx_b (null: n rows), each output that is not null:
//                    img   fp32  dg_normalized_byte - the function k_batch_prep forms its image with
//                    label int64 byte + label_offset, or `fill` without a label plane
//                    mask  fp32 label > 0, or a bool byte label == -1
//                    depth fp32 the byte
//                A plane of a row is H W contiguous bytes, so the lanes walk it flat: lane k of a row owns pixels 4k .. 4k + 3, loads
//                them as ONE 32-bit word per plane (W % 4 == 0 and a 4-byte aligned cache keep every word aligned) and stores 16-byte
//                vectors - a wave's store of a float plane is 1 KiB contiguous - and the bool mask as one 4-byte word.
// No atomics; every byte of every row a put names and every element of every gathered output is written by exactly one lane, so two
// calls give the same bytes.  The row index is read from device memory by every block of the row; one outside [0, n_images) ends the
// block before an address is formed from it.
#include "dg_aux_args.h"
#include "dg_device.h"

#pragma clang fp contract(off)

namespace {
constexpr int TH = DG_BATCH_TH, TW = DG_BATCH_TW;
static_assert(DG_BATCH_THREADS == TH * (TW / 4) && DG_BATCH_THREADS >= TW + TH, "k_batch_prep's tile: one thread per four output pixels");
}  // namespace

// grid (tiles_x * tiles_y, n_records), block 256, 320 bytes of LDS.
__global__ __launch_bounds__(DG_BATCH_THREADS) void k_sc_put(DgSampleCachePutArgs A) {
    __shared__ int s_x[TW], s_y[TH];
    const int tid = threadIdx.x;
    const int32_t* r = A.recs + (size_t)blockIdx.y * DG_BATCH_REC_WORDS;
    const int kind = r[0], n = r[1];
    const size_t src_off = (size_t)(uint32_t)r[2] | ((size_t)(uint32_t)r[3] << 32);
    const int sw = r[4], sh = r[5];
    const int plane = kind == DG_BATCH_IMAGE ? 0 : kind == DG_BATCH_LABEL ? A.label_plane
                    : (kind == DG_BATCH_DEPTH || kind == DG_BATCH_DEPTH_PLANE) ? A.depth_plane : -1;
    if (plane < 0 || n < 0 || n >= A.n) return;     // (the record is uniform over the block: so are this and the barrier below)
    const long long row = A.idx[n];
    if (row < 0 || row >= A.n_images) return;
    const int ty0 = (blockIdx.x / A.tiles_x) * TH, tx0 = (blockIdx.x % A.tiles_x) * TW;

    if (kind != DG_BATCH_DEPTH_PLANE) {
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
    const size_t oplane = (size_t)A.H * A.W;
    uint8_t* dst = A.cache + ((size_t)row * A.planes + plane) * oplane + (size_t)oy * A.W + ox;
    const uint8_t* src = A.packed + src_off;

    if (kind == DG_BATCH_IMAGE) {
        const uint8_t* line = src + (size_t)s_y[ly] * sw * 3;
        uint32_t word[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint8_t* px = line + (size_t)s_x[lx + j] * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) word[c] |= (uint32_t)px[c] << (8 * j);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(dst + c * oplane) = word[c];
    } else {
        uint32_t word = 0xffffffffu;                // DG_BATCH_DEPTH_PLANE: four bytes 255
        if (kind != DG_BATCH_DEPTH_PLANE) {
            const uint8_t* line = src + (size_t)s_y[ly] * sw;
            word = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) word |= (uint32_t)line[s_x[lx + j]] << (8 * j);
        }
        *reinterpret_cast<uint32_t*>(dst) = word;
    }
}

// grid (ceil(H W / 4 / 256), rows), block 256.
__global__ __launch_bounds__(DG_SC_THREADS) void k_sc_gather(DgSampleCacheGatherArgs A) {
    const int j = blockIdx.y;
    const long long row = j < A.n ? A.idx_a[j] : A.idx_b[j - A.n];
    if (row < 0 || row >= A.n_images) return;
    const size_t oplane = (size_t)A.H * A.W;
    const size_t q = ((size_t)blockIdx.x * DG_SC_THREADS + threadIdx.x) * 4;
    if (q >= oplane) return;                        // H W % 4 == 0: a lane has its four pixels or none
    const uint8_t* src = A.cache + (size_t)row * A.planes * oplane + q;
    const size_t opix = (size_t)j * oplane + q;

    if (A.img) {
        uint32_t word[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) word[c] = *reinterpret_cast<const uint32_t*>(src + c * oplane);      // (the three loads are in flight together)
        float* dst = A.img + (size_t)j * 3 * oplane + q;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float m = A.mean[c], s = A.stdv[c];
            *reinterpret_cast<float4*>(dst + c * oplane) =
                make_float4(dg_normalized_byte(word[c] & 0xffu, m, s), dg_normalized_byte((word[c] >> 8) & 0xffu, m, s),
                            dg_normalized_byte((word[c] >> 16) & 0xffu, m, s), dg_normalized_byte(word[c] >> 24, m, s));
        }
    }
    if (A.label || A.mask) {
        long long lab[4] = {A.fill, A.fill, A.fill, A.fill};
        if (A.label_plane >= 0) {
            const uint32_t word = *reinterpret_cast<const uint32_t*>(src + (size_t)A.label_plane * oplane);
#pragma unroll
            for (int k = 0; k < 4; ++k) lab[k] = (long long)((word >> (8 * k)) & 0xffu) + A.label_offset;
        }
        if (A.label) {
            longlong2* dst = reinterpret_cast<longlong2*>(A.label + opix);
            dst[0] = make_longlong2(lab[0], lab[1]);
            dst[1] = make_longlong2(lab[2], lab[3]);
        }
        if (A.mask && A.mask_rule == DG_BATCH_MASK_FLOAT_POSITIVE) {
            *reinterpret_cast<float4*>(static_cast<float*>(A.mask) + opix) =
                make_float4(lab[0] > 0 ? 1.0f : 0.0f, lab[1] > 0 ? 1.0f : 0.0f, lab[2] > 0 ? 1.0f : 0.0f, lab[3] > 0 ? 1.0f : 0.0f);
        } else if (A.mask) {                        // DG_BATCH_MASK_BOOL_IGNORED: torch.bool is one byte, 0 / 1
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) word |= (lab[k] == -1 ? 1u : 0u) << (8 * k);
            *reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(A.mask) + opix) = word;
        }
    }
    if (A.depth) {
        const uint32_t word = *reinterpret_cast<const uint32_t*>(src + (size_t)A.depth_plane * oplane);
        *reinterpret_cast<float4*>(A.depth + opix) =
            make_float4((float)(word & 0xffu), (float)((word >> 8) & 0xffu), (float)((word >> 16) & 0xffu), (float)(word >> 24));
    }
}

hipError_t dg_launch_samplecache_put(const DgSampleCachePutArgs& A, hipStream_t s) {
    return dg_launch_if(false, k_sc_put, dim3(A.tiles_x * A.tiles_y, A.n_records), dim3(DG_BATCH_THREADS), 0, s, A);
}

hipError_t dg_launch_samplecache_gather(const DgSampleCacheGatherArgs& A, hipStream_t s) {
    const size_t lanes = ((size_t)A.H * A.W) / 4;
    const int rows = A.idx_b ? 2 * A.n : A.n;
    return dg_launch_if(false, k_sc_gather, dim3((unsigned)((lanes + DG_SC_THREADS - 1) / DG_SC_THREADS), (unsigned)rows), dim3(DG_SC_THREADS),
                        0, s, A);
}
