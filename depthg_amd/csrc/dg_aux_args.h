// The stand-alone operations (dg_sample, dg_metrics, dg_knn, dg_lhp, dg_optim, dg_attn, dg_linear, dg_augment, dg_batch, dg_feat_cache, dg_sample_cache .hip; dg_api_aux.hip): constants and launchers.
// (The auxiliary loss terms have a header of their own: dg_loss_args.h.)
#pragma once
#include "dg_common.h"

hipError_t dg_launch_salience_coords(const float* sal, int B, int H, int W, int n, const float* u_sel, const float* u_fb,
                                     float* out, hipStream_t s);
hipError_t dg_launch_simple_coords(const float* depth, int B, int H, int W, int h, int w, int n, const float* u_val,
                                   const float* u_pick, float* out, hipStream_t s);
hipError_t dg_launch_confusion(const long long* preds, const long long* target, long long count, int ncls, int nrows,
                               unsigned long long* stats, hipStream_t s);
hipError_t dg_launch_sims_nt(const float* q, const float* x, long long rows_q, long long n, int F, long long q_stride, long long x_stride,
                             float* out, long long out_stride, hipStream_t s);
hipError_t dg_launch_topk_rows(const float* vals, long long rows, long long cols, long long row_stride, int k,
                               long long* out_idx, float* out_val, hipStream_t s);
hipError_t dg_launch_lhp_points(const float* depth, int B, int H, int W, int h, int w, float factor, float* points, hipStream_t s);
hipError_t dg_launch_lhp_propagate(bool backward, const float* src, const float* points, float* stats, int B, int D, int P,
                                   float* dst, hipStream_t s);
hipError_t dg_launch_lhp_map(int mode, const float* code, const float* attn, const float* points, const float* divide, int B, int D,
                             int h, int w, int heads, float* out, float* map, hipStream_t s);
hipError_t dg_launch_lhp_map_bwd(int mode, const float* g, const float* map, const float* divide, int B, int D, int h, int w,
                                 float* gcode, hipStream_t s);

// ---- the optimisation step's Adams as one launch (dg_optim.hip; src/train_segmentation.py:447-455, 537-547)
#define DG_ADAM_MAX_SEGS 16                  // segments (tensors) per launch: dg_adam_step splits longer tables
#define DG_ADAM_MAX_GROUPS 16                // hyper-parameter groups per call
#define DG_ADAM_THREADS 256
#define DG_ADAM_CHUNK (4 * DG_ADAM_THREADS)  // elements per block: one 128-bit access per thread and tensor
// at most DG_ADAM_MAX_SEGS segments; tickets: null, or the first segment's counter (segment k takes tickets[k])
hipError_t dg_launch_adam(const dg_adam_seg* segs, int n_seg, const dg_adam_group* groups, int n_groups, bool device_steps,
                          unsigned int* tickets, hipStream_t s);

// ---- fused attention forward of the frozen ViT (dg_attn.hip; src/dino/vision_transformer.py:80-92)
size_t dg_attn_workspace(int B, int heads, int N);           // bytes of the packed bf16 K / V images
hipError_t dg_launch_attention(const float* qkv, float* out, void* ws, int B, int N, int heads, float scale, hipStream_t s);

// ---- fused cross-attention of the depth guidance, forward and backward (dg_xattn.hip; src/modules.py:524, :566-585)
#define DG_XATTN_HD 48                       // head dimension (384 / 8)
#define DG_XATTN_IMG 7168                    // bytes of one packed tile of 32 rows: 3 row fragments + 4 transposed ones, 1 KiB each
struct DgXattnWs {                           // byte offsets of the workspace's sections (multiples of 256)
    size_t img_k, img_v, img_q, img_do, lse2, di, total;
    int tiles_q, tiles_k;
};
DgXattnWs dg_xattn_ws(int B, int heads, int Nq, int Nk, bool backward);
struct DgXattnArgs {
    const float *q, *k, *v;                  // (B, Nq | Nk, heads * 48)
    const float *out, *lse, *d_out;          // backward: the forward's results and d out
    float *out_w, *lse_w;                    // forward: O, and the log-sum-exp (B, heads, Nq) or null
    float *d_q, *d_k, *d_v;                  // backward: d_q may be null, d_k and d_v only together
    void* workspace;
    int B, heads, Nq, Nk;
    float scale, inv_keep;
    uint64_t seed;
    uint32_t thr;                            // a key is kept iff its Philox word >= thr; 0: no dropout, no generator work
};
hipError_t dg_launch_xattn_forward(const DgXattnArgs& A, hipStream_t s);
hipError_t dg_launch_xattn_backward(const DgXattnArgs& A, hipStream_t s);
hipError_t dg_launch_xattn_mask(uint8_t* out, int B, int heads, int Nq, int Nk, uint64_t seed, uint32_t thr, hipStream_t s);

// ---- fused bf16 linear layers of the frozen ViT (dg_linear.hip; src/dino/vision_transformer.py:49-65, 68-92, 95-115)
bool dg_linear_supported(int K, int Nout);                   // multiples of 64 up to 3072
size_t dg_linear_packed_bytes(int K, int Nout);              // 0 when unsupported
hipError_t dg_launch_linear_pack(const float* w, int K, int Nout, void* packed, hipStream_t s);
hipError_t dg_launch_linear(const void* x, const float* gamma, const float* beta, float eps, const void* packed, const float* bias,
                            const float* residual, void* out, int M, int K, int Nout, int flags, hipStream_t s);

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

// ---- batch preparation: the loader transform of a batch and its positives in one launch (dg_batch.hip; src/utils.py:164-182,
// src/data.py:87-132, 815-912, 1073-1141)
#define DG_BATCH_TH 16                       // output tile: 16 rows x 64 columns, one thread per four neighbouring pixels
#define DG_BATCH_TW 64
#define DG_BATCH_THREADS 256
#define DG_BATCH_REC_WORDS 8                 // 32-bit words of one record (include/depthg_corr.h lists them)
#define DG_BATCH_MAX_SIDE 16384              // of a source plane and of the output
struct DgBatchArgs {
    const uint8_t* packed;                   // the decoded source planes of every sample
    const int32_t* recs;                     // n_records records of DG_BATCH_REC_WORDS words
    const int32_t* tables;                   // per sample xs[W] then ys[H]
    float* img;                              // (N, 3, H, W)
    long long* label;                        // (N, H, W)
    void* mask;                              // (N, H, W): bool bytes or float32, by the label records' rule
    float* depth;                            // (N, H, W)
    int n_records, N, H, W;
    int tiles_x, tiles_y;
    float mean[3], stdv[3];
};
hipError_t dg_launch_batch_prep(const DgBatchArgs& A, hipStream_t s);
// a table entry held inside its plane of n pixels a side (the host entries have checked a host copy of the tables)
__device__ __forceinline__ int dg_hold(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// ToTensor's division, then Normalize's sub and div, on one byte: float32 with IEEE division and no contraction - the bits of torch's
// CPU chain.  k_batch_prep and k_sc_gather both form their image through this one function, so the two cannot drift apart.
__device__ __forceinline__ float dg_normalized_byte(uint8_t b, float mean, float stdv) {
#pragma clang fp contract(off)
    return ((float)b / 255.0f - mean) / stdv;
}

// ---- device-resident sample cache: the loader's output bytes of every image, stored once; a batch and its positives come back in the
// step's dtypes from one launch (dg_sample_cache.hip; src/utils.py:164-182, src/data.py:894-902, :126-128)
#define DG_SC_THREADS 256                    // k_sc_gather: one lane per four neighbouring pixels of a row's planes
#define DG_SC_MAX_ROWS 65535                 // rows per gather call, both lists together (gridDim.y)
struct DgSampleCachePutArgs {
    uint8_t* cache;                          // (n_images, planes, H, W)
    const long long* idx;                    // n cache rows, one per sample
    const uint8_t* packed;                   // the decoded source planes of every sample, as DgBatchArgs
    const int32_t* recs;                     // n_records records of DG_BATCH_REC_WORDS words
    const int32_t* tables;                   // per sample xs[W] then ys[H]
    long long n_images;
    int planes, label_plane, depth_plane;    // a plane the cache lacks: -1
    int n_records, n, H, W;
    int tiles_x, tiles_y;
};
struct DgSampleCacheGatherArgs {
    const uint8_t* cache;
    const long long *idx_a, *idx_b;          // n rows each; idx_b null: n output rows, else 2 n
    float* img;                              // (rows, 3, H, W); any output may be null
    long long* label;                        // (rows, H, W)
    void* mask;                              // (rows, H, W): bool bytes or float32, by mask_rule
    float* depth;                            // (rows, H, W)
    long long n_images;
    int planes, label_plane, depth_plane;
    int n, H, W;
    int label_offset, fill, mask_rule;       // label = byte + label_offset, or `fill` without a label plane
    float mean[3], stdv[3];
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
