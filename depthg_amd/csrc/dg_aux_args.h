// The stand-alone operations (dg_sample, dg_metrics, dg_knn, dg_lhp, dg_optim, dg_attn, dg_linear, dg_xattn .hip; dg_api_aux.hip): constants and launchers.
// (The auxiliary loss terms and the training data path have headers of their own: dg_loss_args.h, dg_data_args.h.)
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
