// The training data path (dg_augment, dg_batch, dg_sample_cache, dg_feat_cache, dg_epoch .hip; dg_api_data.hip): constants, argument blocks and
// launchers, and the device code the loader kernels share - the record decode, the tile prologue, the four-byte gather and the
// four-pixel writers of k_batch_prep, k_sc_put and k_sc_gather.
#pragma once
#include "dg_common.h"

// ---- GPU batch augmentation: img_aug and coord_aug of a batch in two launches (dg_augment.hip; src/data.py:1082-1139,
// src/train_segmentation.py:602-610)
#define DG_AUGM_TH 16                        // output tile: 16 rows x 64 columns, one thread per four neighbouring pixels
#define DG_AUGM_TW 64
#define DG_AUGM_THREADS 256
#define DG_AUGM_STAT_BLOCKS 64               // k_augm_stats: at most this many blocks - and fp64 partials - per image
#define DG_AUGM_REC_WORDS 16                 // 32-bit words of one image's record (include/depthg_corr.h lists them)
#define DG_AUGM_BRIGHTNESS 0                 // op ids of a record's four slots; -1: none
#define DG_AUGM_CONTRAST 1
#define DG_AUGM_SATURATION 2
#define DG_AUGM_HUE 3
struct DgAugmentArgs {
    const float* img;                        // (B, 3, H, W)
    const int32_t* recs;                     // B records of DG_AUGM_REC_WORDS words
    const float *rows, *cols;                // linspace(-1, 1, H), linspace(-1, 1, W)
    float *img_aug, *coord_aug;              // (B, 3, h, w), (B, h, w, 2)
    double* partials;                        // (B, stat_blocks): the gray sums in front of each image's contrast op
    int B, H, W, h, w;
    int tiles_x, tiles_y, stat_blocks;
    int unit_space;                          // 1: the ops act on the tensor as given; 0: x * stdv + mean in front, (x - mean) / stdv behind
    int vec_stores;                          // 1: w % 4 == 0 and both outputs 16-byte aligned
    float mean[3], stdv[3];
};
hipError_t dg_launch_augment(const DgAugmentArgs& A, bool stats, hipStream_t s);

// ---- the loader transform, as batch preparation and the sample cache share it (dg_batch.hip, dg_sample_cache.hip; src/utils.py:164-182,
// src/data.py:87-132, 815-912, 1073-1141)
#define DG_BATCH_TH 16                       // output tile: 16 rows x 64 columns, one thread per four neighbouring pixels
#define DG_BATCH_TW 64
#define DG_BATCH_THREADS 256
#define DG_BATCH_REC_WORDS 8                 // 32-bit words of one record (include/depthg_corr.h lists them)
#define DG_BATCH_MAX_SIDE 16384              // of a source plane and of the output
static_assert(DG_BATCH_THREADS == DG_BATCH_TH * (DG_BATCH_TW / 4), "one thread per four neighbouring output pixels");
static_assert(DG_BATCH_THREADS >= DG_BATCH_TW + DG_BATCH_TH, "the tables of a tile are read by the threads 0 .. TW + TH - 1");
struct DgLoaderSource {                      // what k_batch_prep and k_sc_put read
    const uint8_t* packed;                   // the decoded source planes of every sample
    const int32_t* recs;                     // n_records records of DG_BATCH_REC_WORDS words
    const int32_t* tables;                   // per sample xs[W] then ys[H]
    int n_records, H, W;                     // H x W: the output
    int tiles_x, tiles_y;
};
struct DgLoaderOutputs {                     // what k_batch_prep and k_sc_gather write; k_sc_gather skips a null one
    float* img;                              // (rows, 3, H, W)
    long long* label;                        // (rows, H, W)
    void* mask;                              // (rows, H, W): bool bytes or float32, by the mask rule
    float* depth;                            // (rows, H, W)
    float mean[3], stdv[3];
};
struct DgCachePlanes {                       // a sample cache: uint8 (n_images, planes, H, W)
    long long n_images;
    int planes, label_plane, depth_plane;    // a plane the cache lacks: -1
};

// ---- batch preparation: the loader transform of a batch and its positives in one launch (dg_batch.hip)
struct DgBatchArgs {
    DgLoaderSource src;
    DgLoaderOutputs out;
    int N;
};
hipError_t dg_launch_batch_prep(const DgBatchArgs& A, hipStream_t s);

// ---- device-resident sample cache: the loader's output bytes of every image, stored once; a batch and its positives come back in the
// step's dtypes from one launch (dg_sample_cache.hip; src/utils.py:164-182, src/data.py:894-902, :126-128)
#define DG_SC_THREADS 256                    // k_sc_gather: one lane per four neighbouring pixels of a row's planes
#define DG_SC_MAX_ROWS 65535                 // rows per gather call, both lists together (gridDim.y)
struct DgSampleCachePutArgs {
    uint8_t* cache;
    const long long* idx;                    // n cache rows, one per sample
    DgLoaderSource src;
    DgCachePlanes c;
    int n;
};
struct DgSampleCacheGatherArgs {
    const uint8_t* cache;
    const long long *idx_a, *idx_b;          // n rows each; idx_b null: n output rows, else 2 n
    DgLoaderOutputs out;
    DgCachePlanes c;
    int n, H, W;
    int label_offset, fill, mask_rule;       // label = byte + label_offset, or `fill` without a label plane
};
hipError_t dg_launch_samplecache_put(const DgSampleCachePutArgs& A, hipStream_t s);
hipError_t dg_launch_samplecache_gather(const DgSampleCacheGatherArgs& A, hipStream_t s);

// ---- frozen-backbone feature cache: store image_feat rows once, gather a batch and its positives in one launch (dg_feat_cache.hip;
// src/modules.py:90-137, src/train_segmentation.py:194-212)
#define DG_FC_THREADS 256
#define DG_FC_UNROLL 2                       // 16-byte cache vectors per lane
#define DG_FC_SPAN (DG_FC_THREADS * DG_FC_UNROLL)      // ... and per block
#define DG_FC_MAX_ROWS 65535                 // rows per call (gridDim.y)
#define DG_FC_BF16_NAN 0xFFFFu               // every NaN as bfloat16: what torch's .to(torch.bfloat16) stores for a tensor
hipError_t dg_launch_featcache_put(void* cache, int dtype, long long N, long long L, const float* src, const long long* idx, int n,
                                   hipStream_t s);
// idx_b null: n rows, else 2 n
hipError_t dg_launch_featcache_gather(const void* cache, int dtype, long long N, long long L, const long long* idx_a, const long long* idx_b,
                                      int n, float* out, hipStream_t s);

// ---- the batch draw of a cached step on the device: dataset indices from the epoch's order, kNN positives from Philox, both keyed by
// device memory (dg_epoch.hip; src/data.py:1073-1080)
#define DG_EPOCH_MAX_B 1024                  // one block: a batch of at most this many samples
hipError_t dg_launch_epoch_draw(unsigned long long* state, const long long* order, const long long* nns, int B, int num_neighbors,
                                long long n_images, int K, long long* ind, long long* ind_pos, hipStream_t s);

// ---- the loader kernels' shared device code.  A lane owns four neighbouring pixels of a row and carries their bytes of a plane as one
// 32-bit word, pixel k in bits 8 k .. 8 k + 7: what the cache stores, what the gather loads, what the writers take.
// a table entry held inside its plane of n pixels a side (the host entries have checked a host copy of the tables)
__device__ __forceinline__ int dg_hold(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

struct DgRecord {
    int kind, sample;
    size_t src_off;                          // of the source plane inside `packed`
    int sw, sh, label_offset, mask_rule;
};
__device__ __forceinline__ DgRecord dg_record(const int32_t* recs, int i) {
    const int32_t* r = recs + (size_t)i * DG_BATCH_REC_WORDS;
    return {r[0], r[1], (size_t)(uint32_t)r[2] | ((size_t)(uint32_t)r[3] << 32), r[4], r[5], r[6], r[7]};
}

struct DgTileLane {
    int ly, lx;                              // the lane's row and first column inside the tile
    int oy, ox;                              // ... and inside the output
    bool owns;                               // W % 4 == 0: a lane has its four columns or none
};
// The prologue of a block of grid (tiles_x * tiles_y, records): with `reads` (uniform over the block, as the record is - so is the
// barrier) the tile's 64 column and 16 row indices of the record's sample go to s_x[DG_BATCH_TW] / s_y[DG_BATCH_TH], each held inside the
// source plane.  A block-uniform early return of the caller's stands in front of this call.
__device__ __forceinline__ DgTileLane dg_tile_prologue(const DgLoaderSource& S, const DgRecord& R, bool reads, int* s_x, int* s_y) {
    const int tid = threadIdx.x;
    const int ty0 = (blockIdx.x / S.tiles_x) * DG_BATCH_TH, tx0 = (blockIdx.x % S.tiles_x) * DG_BATCH_TW;
    if (reads) {
        const int32_t* xs = S.tables + (size_t)R.sample * (S.W + S.H);
        const int32_t* ys = xs + S.W;
        if (tid < DG_BATCH_TW) {
            s_x[tid] = tx0 + tid < S.W ? dg_hold(xs[tx0 + tid], R.sw) : 0;
        } else if (tid < DG_BATCH_TW + DG_BATCH_TH) {
            const int k = tid - DG_BATCH_TW;
            s_y[k] = ty0 + k < S.H ? dg_hold(ys[ty0 + k], R.sh) : 0;
        }
        __syncthreads();
    }
    DgTileLane L;
    L.ly = tid / (DG_BATCH_TW / 4); L.lx = (tid % (DG_BATCH_TW / 4)) * 4;
    L.oy = ty0 + L.ly; L.ox = tx0 + L.lx;
    L.owns = L.oy < S.H && L.ox < S.W;
    return L;
}

// the lane's four bytes of the record's source plane through the tile's tables (behind a prologue with `reads`); an RGB plane (HWC) has
// step 3 and a channel c
__device__ __forceinline__ uint32_t dg_gather4(const DgLoaderSource& S, const DgRecord& R, const int* s_x, const int* s_y, const DgTileLane& L,
                                               int step = 1, int c = 0) {
    const uint8_t* line = S.packed + R.src_off + (size_t)s_y[L.ly] * R.sw * step + c;
    uint32_t word = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= (uint32_t)line[(size_t)s_x[L.lx + j] * step] << (8 * j);
    return word;
}

// ToTensor's division, then Normalize's sub and div, on one byte: float32 with IEEE division and no contraction - the bits of torch's
// CPU chain.
__device__ __forceinline__ float dg_normalized_byte(uint8_t b, float mean, float stdv) {
#pragma clang fp contract(off)
    return ((float)b / 255.0f - mean) / stdv;
}
// img: three words -> the lane's float4 of each colour plane (dst: the red one's; `oplane` elements to the next)
__device__ __forceinline__ void dg_write_image(float* dst, size_t oplane, const uint32_t word[3], const float* mean, const float* stdv) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = mean[c], s = stdv[c];
        *reinterpret_cast<float4*>(dst + c * oplane) =
            make_float4(dg_normalized_byte(word[c] & 0xffu, m, s), dg_normalized_byte((word[c] >> 8) & 0xffu, m, s),
                        dg_normalized_byte((word[c] >> 16) & 0xffu, m, s), dg_normalized_byte(word[c] >> 24, m, s));
    }
}
// ToTargetTensor and the dataset's offset: label = byte + offset
__device__ __forceinline__ void dg_labels(uint32_t word, int offset, long long lab[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) lab[k] = (long long)((word >> (8 * k)) & 0xffu) + offset;
}
// label: four values as two 16-byte stores, and their mask by `mask_rule` - each unless its pointer is null; opix: the lane's first element
__device__ __forceinline__ void dg_write_label(long long* label, void* mask, size_t opix, int mask_rule, const long long lab[4]) {
    if (label) {
        longlong2* dst = reinterpret_cast<longlong2*>(label + opix);
        dst[0] = make_longlong2(lab[0], lab[1]);
        dst[1] = make_longlong2(lab[2], lab[3]);
    }
    if (!mask) return;
    if (mask_rule == DG_BATCH_MASK_FLOAT_POSITIVE) {
        *reinterpret_cast<float4*>(static_cast<float*>(mask) + opix) =
            make_float4(lab[0] > 0 ? 1.0f : 0.0f, lab[1] > 0 ? 1.0f : 0.0f, lab[2] > 0 ? 1.0f : 0.0f, lab[3] > 0 ? 1.0f : 0.0f);
    } else {                                    // DG_BATCH_MASK_BOOL_IGNORED: torch.bool is one byte, 0 / 1
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) word |= (lab[k] == -1 ? 1u : 0u) << (8 * k);
        *reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(mask) + opix) = word;
    }
}
// depth: the byte values as one float4
__device__ __forceinline__ void dg_write_depth(float* dst, uint32_t word) {
    *reinterpret_cast<float4*>(dst) =
        make_float4((float)(word & 0xffu), (float)((word >> 8) & 0xffu), (float)((word >> 16) & 0xffu), (float)(word >> 24));
}
