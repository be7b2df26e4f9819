// The segmentation head and the probes (dg_head.hip, dg_probe.hip; dg_api_head.hip): argument blocks, the backward's plan, launchers.
#pragma once
#include "dg_common.h"

// ---- the segmentation head (dg_head.hip; DinoFeaturizer's cluster1 / cluster2, src/modules.py:75-88, 122-137)
struct DgHeadFwdArgs {
    const float* feat;                     // (B,C,P) fp32
    const float* w1; const float* b1;      // (D,C), (D)
    const float* w2a; const float* b2a;    // (C,C), (C)   null: projection_type "linear"
    const float* w2b; const float* b2b;    // (D,C), (D)
    const __bf16* w1_bf; const __bf16* w2a_bf; const __bf16* w2b_bf;   // bf16 copies of the three weight matrices (k_head_prep)
    const float* keep1; const float* keep2; const float* keep3;   // (B,C): 1 keep / 0 drop; null: no dropout for that use
    float scale;                           // 1/(1-p) applied where a keep mask is given
    float* code;                           // (B,D,P)
    float* feats_out;                      // (B,C,P) = f * keep3 * scale, or null
    __bf16* hidden;                        // (B,C,P) bf16: ReLU output saved for the backward, or null
    int32_t B, C, D, P;
    unsigned long long* stamps;            // developer timing stamps (null in production)
    // two passes of the featurizer in one launch (dg_head_forward with feat_pos: img, then img_pos): images Bs.. of feat / code / feats_out
    // live in a second tensor each; d_* = (its base - the first's base) in elements - Bs images, added to the offset of those images
    int32_t Bs;
    long long d_feat, d_code, d_fo;
};
// element offset of image b of a tensor that continues in a second allocation from image Bs on (see DgHeadFwdArgs)
__host__ __device__ inline long long dg_img_off(int b, long long stride, int Bs, long long delta) { return (long long)b * stride + (b >= Bs ? delta : 0); }

struct DgHeadDhArgs {
    const float* gcode;      // (B,D,P) fp32
    const __bf16* w2bT;      // (C, DP) bf16: W2b transposed, DP = D rounded up to 32, zero padded (k_head_prep)
    const __bf16* hidden;    // (B,C,P)
    __bf16* dh;              // (B,C,P) out
    float* part_bd;          // [B * tiles][D] per-block row sums of d code (bias gradients of the output convolutions)
    float* part_b2a;         // [B * tiles][C] per-block row sums of d hidden_pre
    int32_t B, C, D, P;
    int32_t Bs; long long d_gcode;   // (pair: images Bs.. of gcode in a second tensor, as DgHeadFwdArgs)
    __bf16* gcode_bf;                // (B,D,P) out or null: d code rounded to bf16, the A2h operand of k_head_wgrad3 (P a multiple of 4)
    int32_t step_major;              // 1 (k_head_dh2 in front of k_head_wgrad3): dh and gcode_bf as [image][step of 32 positions][row][32] - the rows of a step
                                     //    contiguous, what k_head_wgrad3's DMA pieces read (row-major gave them 64-byte pieces of 16 rows: 54 against 45 us)
    float* part_w2b;                 // [blocks][D][C] or null: k_head_dh2 also forms d W2b = d code x hidden^T (both tiles are in its LDS), one partial sum per block
    unsigned long long* stamps;      // developer timing stamps (null in production)
    int32_t staged;                  // (set by the launcher) 1: hidden / d hidden through an LDS image of whole rows (P a multiple of 8)
};

struct DgHeadWgradArgs {
    const void* A; const void* Bm;     // (B, M, P), (B, N, P); fp32 or bf16 (template)
    const float* keep;                 // (B, N) or null
    float* part;                       // [splits][M][N]
    int32_t B, M, N, P, splits;
    // optional second product with the same Bm in the same launch (M2 > 0): A2 (B, M2, P) fp32, its keep mask and partial sums
    const void* A2; const float* keep_2; float* part2; int32_t M2;
    const void* A2h;                   // (B, M2, P) bf16 copy of A2 in ONE tensor (k_head_dh) or null; with it the two products run as k_head_wgrad3
    int32_t a_step_major;              // k_head_wgrad3: A and A2h are [image][step of 32 positions][row][32] (k_head_dh2 wrote them so)
    int32_t Bs; long long dA, dB, dA2;   // (pair: images Bs.. of A / Bm / A2 in second tensors, offsets in their elements; 0: one tensor)
};

hipError_t dg_launch_head_fwd(const DgHeadFwdArgs& a, hipStream_t s);
hipError_t dg_launch_head_prep(const float* w1, const float* w2a, const float* w2b, void* scratch, int C, int D, hipStream_t s);
// The bf16 copies of the head's weights (k_head_prep -> k_head_fwd / k_head_dh*).  The three matrices the forward multiplies with are
// stored FRAGMENT-MAJOR: [16-row block][k-step of 32][lane = 16 (k / 8 % 4) + row % 16][8 bf16] - the 1 KiB a wave reads for one A
// fragment is contiguous (whole cache lines), where row-major copies gave every lane 16 bytes of 16 different rows: 64-byte pieces,
// the rate of which set the forward's k-loop (round 6).  Rows are padded to whole blocks (cluster1 / cluster2's output convolution:
// eight blocks = 128 rows, the most the forward's waves walk), channels to the forward's padded width CP; the padding is zeros.
__host__ __device__ inline int dg_head_cp(int C) { return C <= 64 ? 64 : (C <= 128 ? 128 : (C <= 192 ? 192 : (C <= 384 ? 384 : 768))); }
struct DgHeadWeightLayout {
    int CP, KS; size_t w1, w2a, w2b, w2bT, elems;          // offsets / total in bf16 elements
    __host__ __device__ DgHeadWeightLayout(int C, int D) {
        CP = dg_head_cp(C); KS = CP / 32;
        const size_t blk = (size_t)KS * 512;                // elements of one 16-row block
        w1 = 0; w2a = 8 * blk; w2b = w2a + (size_t)(CP / 16) * blk; w2bT = w2b + 8 * blk;
        elems = w2bT + (size_t)C * ((D + 31) / 32 * 32);
    }
};
// The backward's plan: the workspace carved for a shape AND the kernels that will run on it, decided once, next to the kernels
// (dg_head.hip dg_head_plan).  The launchers below take the route from it; one they cannot run is hipErrorInvalidValue.
enum DgHeadDhRoute { DG_HEAD_DH_TILES,           // k_head_dh, one block per 64-position tile; d W2b is a weight-gradient launch of its own
                     DG_HEAD_DH_FUSED };         // k_head_dh2 on dh_blocks resident blocks; d W2b rides in it (DgHeadDhArgs.part_w2b)
enum DgHeadWgradForm { DG_HEAD_WGRAD_DIRECT,     // k_head_wgrad, one product per launch
                       DG_HEAD_WGRAD_GROUPED,    // k_head_wgrad2 (P and the splits multiples of 8)
                       DG_HEAD_WGRAD_ONE_PASS }; // k_head_wgrad3: d W2a and d W1 in one pass over the features, d code as DgHeadWgradArgs.A2h
struct DgHeadPlan {
    size_t dh, p2a, p1, p2b, pbd, pb2a, gbf, total;      // workspace offsets (gbf: only with DG_HEAD_WGRAD_ONE_PASS), its size
    int s2a, s1, s2b, tiles, dh_blocks;                  // splits of the d W2a + d W1 launch, of d W1 alone, of d W2b; tiles per image
    DgHeadDhRoute dh_route;
    DgHeadWgradForm wgrad_pair, wgrad_single;            // d W2a + d W1 in one call (s2a splits); a product alone (s1 splits: d W1 of the linear head, d W2b)
    bool step_major;                                     // d hidden (and A2h) as DgHeadDhArgs.step_major: k_head_dh2 writes what k_head_wgrad3 reads
};
DgHeadPlan dg_head_plan(int B, int C, int D, int P);
hipError_t dg_launch_head_dh(const DgHeadDhArgs& a, const DgHeadPlan& plan, hipStream_t s);
// a_bf16 / b_bf16: element types of A and Bm - the three pairings the backward uses: fp32 x fp32, fp32 x bf16, and bf16 x fp32 with the
// second product (a.M2 > 0)
hipError_t dg_launch_head_wgrad(const DgHeadWgradArgs& a, DgHeadWgradForm form, bool a_bf16, bool b_bf16, hipStream_t s);
// ---- d image_feat (k_head_dx; opt-in, behind dg_head_backward on the same workspace): per image one product [W1^T | W2a^T] x [g ; dh]
// The transposed bf16 weight copies (k_head_dx_prep), fragment-major as the forward's: [16-row block of image_feat channels][k-step of
// 32 rows of g, then of dh][lane][8 bf16].  Rows are padded to whole passes of the kernel's four waves x MB blocks, g's rows to KS1
// steps and dh's to KS2 (0: linear head); the padding is zeros.
__host__ __device__ inline int dg_head_dx_mb(int C) { return C <= 64 ? 1 : (C <= 128 ? 2 : (C <= 192 ? 3 : (C <= 256 ? 4 : 6))); }
struct DgHeadDxLayout {
    int MB, rows, KS1, KS2; size_t elems;
    __host__ __device__ DgHeadDxLayout(int C, int D, bool nonlinear) {
        MB = dg_head_dx_mb(C);
        rows = (C + 64 * MB - 1) / (64 * MB) * (64 * MB);
        KS1 = (D + 31) / 32; KS2 = nonlinear ? (C + 31) / 32 : 0;
        elems = (size_t)(rows / 16) * (KS1 + KS2) * 512;
    }
};
struct DgHeadDxArgs {
    const float* gcode;              // (B,D,P) fp32, rounded to bf16 on load
    const __bf16* dh;                // d hidden as dg_head_backward left it in its workspace (all B images), or null: linear head
    const __bf16* wT;                // DgHeadDxLayout
    const float* keep1; const float* keep2;   // (B,C) or null
    float scale;
    float* dx; float* dx2;           // (Bs,C,P) out: images 0 .. Bs - 1, and (B - Bs,C,P): images Bs ..; one of a pair may be null (b0 / nb skip it)
    int32_t B, C, D, P;
    int32_t Bs; long long d_gcode;   // (pair: images Bs.. of gcode in a second tensor, as DgHeadFwdArgs)
    int32_t b0, nb;                  // the images this launch computes: b0 .. b0 + nb - 1
    int32_t step_major;              // layout of dh (DgHeadDhArgs.step_major)
    // the epilogue addend (k_head_dx<MB, true>; last: the other fields keep their offsets): d loss / d feats_out (Bs,C,P) per pass, either
    // null, and the (B,C) keep flags of that Dropout2d (null: no mask); dx += scale keep3 gfeats
    const float* gfeats; const float* gfeats2; const float* keep3;
};
hipError_t dg_launch_head_dx_prep(const float* w1, const float* w2a, void* wT, int C, int D, hipStream_t s);
hipError_t dg_launch_head_dx(const DgHeadDxArgs& a, hipStream_t s);

struct DgHeadReduceJob { const float* part; float* out; float* out2; int32_t n, splits; float scale; };
struct DgHeadReduceArgs { DgHeadReduceJob jobs[6]; int32_t njobs; };
hipError_t dg_launch_head_reduce(const DgHeadReduceArgs& a, hipStream_t s);
hipError_t dg_launch_head_rowsum(const void* X, bool bf16, float* out, float* out2, int B, int R, int P, hipStream_t s, int Bs = 1 << 30, long long dX = 0);

// ---- the probes (dg_probe.hip; ClusterLookup src/modules.py:647-675, linear-probe loss src/train_segmentation.py:421-434)
struct DgClusterArgs {
    const float* x;          // (B, D, P)
    const float* clusters;   // (n, D)
    float alpha;             // NaN: hard assignment (alpha is None)
    float* inner;            // (B, n, P) out
    float* probs;            // (B, n, P) out, or null
    float* logp;             // (B, n, P) out: log_softmax(alpha * inner), or null
    float* part;             // [blocks] partial sums of sum_n probs * inner
    int32_t B, D, n, P;
};

struct DgClusterBwdArgs {
    const float* x; const float* clusters; const float* inner;   // as the forward
    const float* gloss;      // [1] upstream gradient of the loss (device)
    float alpha;
    float* dinner;           // (B, n, P) scratch out: d loss / d inner
    float* grad_x;           // (B, D, P) out or null
    float* part;             // [B * ceil(P/64)][n][D] partial sums of d loss / d normalised centres
    float* grad_clusters;    // (n, D) out
    int32_t B, D, n, P;
};

struct DgProbeCeArgs {
    const float* logits;     // (B, n, h, w) the probe's output at feature resolution
    const int64_t* label;    // (B, H, W)
    float* part;             // [B * H][2]: per label row, sum of -log p[label] over the labelled pixels, their count
    const float* gloss;      // backward: [1] upstream of the loss
    const float* total;      // backward: [2] = {loss sum, count} of the forward
    float* grad_logits;      // backward: (B, n, h, w)
    int32_t B, n, h, w, H, W;
};

hipError_t dg_launch_cluster_fwd(const DgClusterArgs& a, float* loss_out, hipStream_t s);
hipError_t dg_launch_cluster_bwd(const DgClusterBwdArgs& a, hipStream_t s);
hipError_t dg_launch_probe_ce_fwd(const DgProbeCeArgs& a, float* out3, hipStream_t s);
hipError_t dg_launch_probe_ce_bwd(const DgProbeCeArgs& a, hipStream_t s);

// ---- the fused probe step (dg_probe_step.hip; both probes of src/train_segmentation.py:421-444 on the detached code, their
// parameter gradients formed in the forward)
struct DgProbeStepArgs {
    const float* code;       // (B, D, h, w), detached
    const int64_t* label;    // (B, H, W)
    const float* lin_w;      // (n, D) the linear probe's 1 x 1 convolution
    const float* lin_b;      // (n) or null
    const float* clusters;   // (m, D) the cluster probe's centres
    float* ws;               // the workspace (DgProbeStepPlan)
    float* out3;             // [3] = {linear loss, cluster loss, labelled pixels}
    int32_t B, D, n, m, h, w, H, W;
};
// The workspace's sections (offsets in floats, each a multiple of 4) and the launches' grids and LDS, for one shape.  P = h w, R = n + m.
//   logits (B,n,P)  the linear probe at feature resolution            ptop, pbot (B,n,P)  the unscaled d logits a feature row receives
//   inv, arg (B,P)  1 / |code| and the winning centre (int32)         from the label rows whose upper tap is that row / the row above
//   part_pos [chunks]  the position pass's partial cluster losses     part_lab [B h][2]  per (image, feature row): loss sum, count (int32)
//   part_red [splits][R][D + 1] doubles  the reduction pass's partial products
//   grads [n D + n + m D] doubles  d W, d b, d clusters for upstream gradients of 1: what the backward scales
struct DgProbeStepPlan {
    size_t o_logits, o_ptop, o_pbot, o_inv, o_arg, o_part_pos, o_part_lab, o_part_red, o_grads, floats;
    int32_t R4, DC4, cpi, chunks, splits, smem_pos, smem_label, smem_reduce;     // cpi: 64-position chunks per image
    __host__ __device__ float* logits(float* ws) const { return ws + o_logits; }
    __host__ __device__ float* ptop(float* ws) const { return ws + o_ptop; }
    __host__ __device__ float* pbot(float* ws) const { return ws + o_pbot; }
    __host__ __device__ float* inv(float* ws) const { return ws + o_inv; }
    __host__ __device__ int32_t* arg(float* ws) const { return reinterpret_cast<int32_t*>(ws + o_arg); }
    __host__ __device__ float* part_pos(float* ws) const { return ws + o_part_pos; }
    __host__ __device__ float* part_lab(float* ws) const { return ws + o_part_lab; }
    __host__ __device__ double* part_red(float* ws) const { return reinterpret_cast<double*>(ws + o_part_red); }
    __host__ __device__ double* grads(float* ws) const { return reinterpret_cast<double*>(ws + o_grads); }
};
// null: the shape is served and `pl` is filled; else the reason it is refused (nothing is launched)
const char* dg_probe_step_plan(int B, int D, int n, int m, int h, int w, int H, int W, DgProbeStepPlan& pl);
hipError_t dg_launch_probe_step_fwd(const DgProbeStepArgs& a, const DgProbeStepPlan& pl, hipStream_t s);
hipError_t dg_launch_probe_step_bwd(const float* ws, const DgProbeStepPlan& pl, const float* g_lin, const float* g_clu, int D, int n, int m,
                                    float* gw, float* gb, float* gc, hipStream_t s);
