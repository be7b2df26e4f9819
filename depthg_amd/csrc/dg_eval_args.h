// Evaluation (dg_eval.hip, dg_crf.hip, dg_crf_sort.hip; dg_api_eval.hip): the probes' predictions, dense-CRF refinement and their launchers.
#pragma once
#include "dg_common.h"

// ---- the probes' predictions and confusion counts (dg_eval.hip; src/train_segmentation.py:471-499, src/eval_segmentation.py:146-170)
struct DgSegArgs {
    const float* code;       // (B, D, h, w)
    const float* code_flip;  // (B, D, h, w) second pass on the mirrored image, or null
    const float* lin_w;      // (n, D)
    const float* lin_b;      // (n) or null
    const float* clusters;   // (m, D)
    const int64_t* label;    // (B, H, W)
    float* scores;           // scratch (B, h*w, Kp): Kp = n4 + m4 (each part rounded up to 4), linear rows at 0, cluster rows at n4
    int64_t* stats_lin;      // (n, n) or null
    int64_t* stats_clu;      // (m, n) or null (rows >= n are never touched)
    int64_t* preds_lin;      // (n_store, H, W) or null
    int64_t* preds_clu;      // (n_store, H, W) or null
    int32_t B, D, h, w, n, m, H, W, n_store;
};
#define DG_SEG_MAX_D 1024
#define DG_SEG_MAX_K 256                     // n + m
#define DG_SEG_ROW_FLOATS 16384              // w * Kp: one vertically blended score row in LDS
__host__ __device__ inline int dg_seg_kp(int n, int m) { return (n + 3) / 4 * 4 + (m + 3) / 4 * 4; }
hipError_t dg_launch_segment_predict(const DgSegArgs& a, hipStream_t s);
hipError_t dg_launch_seg_project(const DgSegArgs& a, hipStream_t s);   // k_seg_project alone: a.scores (also dg_crf.hip)
int dg_cu_count();                                                     // compute units of the current device (dg_eval.hip)

// ---- label-free inference (dg_seg_labels.hip; src/demo_segmentation.py:59-78): byte label maps and painted images of both probes.
// (Its kernels live beside dg_eval.hip, not in it: tests/test_eval_cpu.py pins that unit's kernels at the four of the scored route.)
struct DgPaintArgs {
    const int32_t* remap;    // (m) cluster id -> class id (-1 -> 255), or null: the raw cluster id
    const float* img;        // (B, 3, H, W) normalised, or null (alpha256 == 256, or no colour output)
    const uint8_t* cmap;     // (cmap_rows, 3), or null (no colour output)
    uint8_t* lab_lin;        // (B, H, W) or null
    uint8_t* lab_clu;        // (B, H, W) or null
    uint8_t* rgb_lin;        // (B, H, W, 3) or null
    uint8_t* rgb_clu;        // (B, H, W, 3) or null
    float mean[3], std[3];   // pix = clamp(rint((img * std + mean) * 255), 0, 255)
    int32_t B, H, W, m, cmap_rows, alpha256;
};
#define DG_SEG_MAX_LABELS 255                // n and m of the byte maps: 255 is the "no class" byte
#define DG_SEG_MAX_CMAP 256
#define DG_SEG_STAGE_BYTES (64 * 1024)       // LDS staging of a chunk's output bytes (8 per pixel and 16 of slack per output)
hipError_t dg_launch_segment_labels(const DgSegArgs& a, const DgPaintArgs& p, hipStream_t s);   // a.scores: the projection scratch
hipError_t dg_launch_label_paint(const int64_t* preds, int G, const DgPaintArgs& p, hipStream_t s);

// ---- dense-CRF refinement (dg_crf.hip; src/crf.py dense_crf, src/eval_segmentation.py:55-60, :162-167)
#define DG_CRF_MAX_GROUPS 8                  // channel groups (one softmax each: one per probe)
#define DG_CRF_MAX_KP 256                    // channels, each group rounded up to a multiple of 4
#define DG_CRF_MAX_HW (1 << 24)              // pixels of one image
// The packing of one permutohedral lattice's vertex keys into 64 bits: the first d coordinates of a vertex, each biased by lo[i] and
// given bits[i] bits, coordinate 0 highest; the image of the chunk above them (bits kbits and up).
struct DgCrfKeys {
    int32_t d;                // feature dimension: 2 (Gaussian: x, y) or 5 (bilateral: x, y, B, G, R)
    float stdv[5];            // the features are (x, y, B, G, R)[i] / stdv[i]
    float scale[5];           // elevation scale of feature i: sqrt(2/3) (d + 1) / sqrt((i + 1)(i + 2))
    int32_t lo[5], shift[5];
    int32_t kbits;            // sum of the coordinates' bits
};
bool dg_crf_key_plan(int d, int H, int W, const float* stdv, DgCrfKeys& k);       // false: the key range does not fit 64 bits
int dg_crf_max_chunk(const DgCrfKeys& k);                                         // images one packed key range can hold
#define DG_CRF_GAUSSIAN 1                    // lattice masks of dg_crf_chunk_bytes / dg_crf_workspace_bytes
#define DG_CRF_BILATERAL 2
size_t dg_crf_chunk_bytes(int c, int H, int W, int Kp, int lats);                 // workspace of a chunk of c images, 0: refused
struct DgCrfArgs {
    const float* img;         // (B, 3, H, W) normalised (the loader's T.Normalize), or null (Gaussian filter only)
    const float* in;          // dg_crf_filter: values (B, C, H, W); dg_dense_crf: the unary U (B, C, H, W)
    float* out;               // dg_crf_filter: the message (B, C, H, W); dg_dense_crf: Q (B, C, H, W) or null
    int64_t* preds;           // dg_dense_crf: (G, B, H, W) arg-max within each group, or null
    void* ws;
    size_t ws_bytes;
    int32_t B, C, H, W, G, Kp;
    int32_t gend[DG_CRF_MAX_GROUPS];   // group g: channels [gend[g-1], gend[g]); its padded columns start at goff[g]
    int32_t goff[DG_CRF_MAX_GROUPS];
    int32_t n_iter;
    float w_pos, w_bi;        // Potts weights (POS_W, Bi_W)
    DgCrfKeys kg, kb;         // the Gaussian and the bilateral lattice
    int32_t filter_bilateral; // dg_crf_filter: which kernel
};
hipError_t dg_launch_crf_filter(const DgCrfArgs& a, hipStream_t s);
hipError_t dg_launch_dense_crf(const DgCrfArgs& a, hipStream_t s);
hipError_t dg_launch_crf_unary(const float* logits, int B, int C, int h, int w, int H, int W, int G, const int32_t* gend, float* U,
                               hipStream_t s);
hipError_t dg_launch_segment_unary(const DgSegArgs& a, float alpha, float* U, hipStream_t s);   // a.scores: the projection scratch
// rocPRIM's device-wide radix sort and scan (dg_crf_sort.hip)
size_t dg_crf_sort_temp_bytes(int n);
hipError_t dg_crf_sort_pairs(void* temp, size_t temp_bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout,
                             int n, int bits, hipStream_t s);
hipError_t dg_crf_scan(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int n, hipStream_t s);
