/*
 * depthg_corr.h - C ABI of the MI355X (gfx950) implementation of DepthG's feature-correlation
 * loss hot path.  Plain C: pointers and sizes only, no torch types.
 *
 * The reference (leonsick/depthg) has no FFI; the boundary it offers for this path is the
 * Python nn.Module `ContrastiveCorrelationLoss` (src/modules.py:1221-1367).  The host-side
 * mirror of that module lives in depthg_amd/loss.py and binds these entry points with ctypes
 * (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller unless stated otherwise;
 *  - the callee never allocates or frees: scratch comes from a caller-sized workspace whose
 *    size is returned by dg_corr_workspace_bytes();
 *  - every launch goes to the given hipStream_t and is asynchronous w.r.t. the host;
 *  - return value 0 = ok, negative = error (dg_last_error() gives text); no exceptions.
 *  - one host thread per device; state kept across calls: the thread-local last-error string and a per-kernel cache of the
 *    dynamic-LDS attribute.
 */
#ifndef DEPTHG_CORR_H
#define DEPTHG_CORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_VERSION 119   /* 119: one entry per operation where a NULL pointer already told the variants apart - dg_head_forward / dg_head_backward / dg_head_backward_input take the second pass's tensors (NULL: one pass) and the input gradient its optional feats_out addend, dg_fps_coords takes depth_pos, dg_super_perms takes keys, seed and state; the eight entries these replace are gone, nothing is computed differently; 118: dg_corr_forward_intra_feats + dg_corr_workspace_bytes_intra_feats, dg_corr_cd_hist, the three dg_crfloss the three dg_augalign entry points and dg_batch_prep (more exports under the same number: the layouts and meanings of every earlier entry point are unchanged, and a binding that declares a new symbol refuses a library without it when it loads), dg_sampled_sumsq, dg_corr_forward_extnorm (feature maps wider than 768 channels on SAMPLED grids above 160 positions, in channel chunks); 117: DG_FEATS_UNIT, dg_normalize_split (feature maps wider than 768 channels on the dense identity grid, in chunks of the width the operand kernels hold: the loss is linear in the feature correlation); 116: dg_prof_main_span takes FOUR words (+ the workgroups' lifetimes in shader cycles and wall ticks: the clock the CUs held); 115: dg_corr_intra_folded; 114: the two-tensor FPS call takes a workspace (dg_fps_workspace_bytes(2 B, h, w): the pooled depth maps, written by a launch over the whole chip in front of the sampler), dg_corr_materialize_shared, dg_prof_main_span (the fused correlation launch's execution span inside a replayed step), sample grids of <= 160 positions at any feature width (fused small-grid kernel); 113: dg_corr_forward_masked; 112: dg_rand_coords_state; 111: the head on both featurizer passes in one set of launches; 110: FPS on both depth tensors in one launch; 109: dg_knn_similarities; 108: dg_corr_desc.code_h / code_w (code maps of another resolution than the feature maps: the FeaturePyramidNet producer, src/modules.py:732-766), dg_corr_desc.flags DG_EXACT_MASKS; 107: dg_head_*, dg_cluster_lookup_*, dg_probe_ce_*; 106: dg_corr_main_kernel_name; 105: dg_corr_forward_draw; 104: dg_lhp_map_forward / dg_lhp_map_backward; 103: super_perms from a device-resident generator state; 102: DG_LINE_GRID, dg_salience_coords, dg_simple_depth_coords; 101: total weights, DG_OUT_TOTAL */

/* flags of dg_corr_desc.flags (names follow the cfg keys read at src/modules.py:1236-1352) */
#define DG_POINTWISE      (1u << 0)  /* cfg.pointwise: spatial centering of fd (modules.py:1236-1239) */
#define DG_ZERO_CLAMP     (1u << 1)  /* cfg.zero_clamp: clamp min 0 instead of -9999 (modules.py:1243-1246) */
#define DG_STABALIZE      (1u << 2)  /* cfg.stabalize: clamp max 0.8 (modules.py:1249-1250) */
#define DG_DEPTH_TERM     (1u << 3)  /* cfg.depth_feat_correlation_loss (modules.py:1334-1336) */
#define DG_NEED_GRAD      (1u << 4)  /* also produce d/d orig_code, d/d orig_code_pos pieces */
#define DG_SHARED_COORDS  (1u << 5)  /* coords1[n] == coords2[m] for all n, m (dense grid): negatives reuse
                                        the prepared operand of `feats`/`code` through the batch permutation */

#define DG_IDENTITY_GRID  (1u << 6)  /* with DG_SHARED_COORDS and S == h == w: both coords are the pixel-centre grid
                                        (coords[b,u,v] = (lin[v], lin[u]), lin = linspace(-1,1,S)): sample() is an exact
                                        transpose and the feats operands are built without bilinear taps */

#define DG_LINE_GRID      (1u << 7)  /* the sample grid is S x 1 instead of S x S: coords are (B,S,1,2), P = S positions and the
                                        un-reduced tensors are (B,1,S,1,S) - what depth_sampling='simple' feeds the loss
                                        (simple_depth_informed_sampling returns (B,n,1,2), src/modules.py:828-883,1299-1302);
                                        the depth term resizes depth to (1,S) (modules.py:1261-1262 with c1.shape[2:] = (1,S)) */

#define DG_EXACT_MASKS    (1u << 8)  /* build-side cfg key `dg_exact_masks`: on a gradient pass of the zero_clamp recipe the clamp mask
                                        1[cd >= 0] (modules.py:1250-1252) is decided by an fp32 cd wherever the fp16 cd the MFMAs
                                        compute is too close to zero to be trusted; without the flag the fp16 cd decides on the
                                        dense grids (the small sample grids always take exact masks) */

#define DG_FEATS_UNIT     (1u << 9)  /* with DG_IDENTITY_GRID: the channel vectors of orig_feats / orig_feats_pos are used as they are, not
                                        normalised - they are unit vectors already, or ONE CHANNEL CHUNK of unit vectors
                                        (dg_normalize_split).  The loss and its gradients are linear in the feature correlation
                                        fd (src/modules.py:797-809, 1231-1254: centering, shift and clamp(cd) * (fd - shift)), and fd is
                                        a sum over channels: a map of C > 768 channels is evaluated as one call per chunk - the first
                                        with the recipe's shifts and depth term, the others with zero shifts and no depth term - and
                                        the loss means (not the cd means) and code gradients add up (depthg_amd/loss.py does that). */
#define DG_MAX_NEG 8

/* error codes */
#define DG_OK               0
#define DG_ERR_INVALID     -1
#define DG_ERR_UNSUPPORTED -2
#define DG_ERR_WORKSPACE   -3
#define DG_ERR_LAUNCH      -4

typedef void* dg_stream_t; /* hipStream_t */

/* Shape/cfg descriptor of one loss call (one `ContrastiveCorrelationLoss.forward`). */
typedef struct dg_corr_desc {
    int32_t B;        /* batch (per rank) */
    int32_t C;        /* feature channels of orig_feats (384 ViT-S, 768 ViT-B); <= 768 per call on grids above 160 positions and the identity grid
                         (wider maps: one call per channel chunk - DG_FEATS_UNIT on the identity grid, dg_corr_forward_extnorm on sampled
                         coordinates), <= 8192 on smaller grids */
    int32_t D;        /* code channels = cfg.dim; <= 128 */
    int32_t h, w;     /* feature-map size of orig_feats / orig_feats_pos (and of the code maps unless code_h / code_w say otherwise) */
    int32_t S;        /* cfg.feature_samples; P = S*S positions are correlated (P = S with DG_LINE_GRID) */
    int32_t n_neg;    /* cfg.neg_samples (<= DG_MAX_NEG) */
    int32_t depth_h, depth_w; /* size of the depth map (image resolution); 0 if no depth */
    uint32_t flags;
    float shift_intra, shift_inter, shift_neg, shift_depth; /* cfg.pos_intra_shift ... cfg.depth_feat_shift */
    /* weights of the four loss means in the caller's total (src/train_segmentation.py:330-349: cfg.pos_intra_weight,
       pos_inter_weight, neg_inter_weight, depth_feat_weight, each times correspondence_weight - balance);
       out_scalars[DG_OUT_TOTAL] = their weighted sum.  All zero: no total wanted. */
    float w_intra, w_inter, w_neg, w_depth;
    /* size of orig_code / orig_code_pos when it differs from (h, w); 0, 0 = the same maps.  The reference's sample()
       (src/modules.py:822-825) takes normalised coordinates, so the loss accepts producers whose code map has another resolution
       than their feature map: FeaturePyramidNet returns low_res_feats (B,2048,7,7) next to code (B,dim,56,56), src/modules.py:732-766
       (its 2048 feature channels exceed this library's C <= 768).  Needs general coordinates (no DG_IDENTITY_GRID). */
    int32_t code_h, code_w;
} dg_corr_desc;

/* indices into out_scalars[] of dg_corr_forward */
enum {
    DG_OUT_LOSS_INTRA = 0, /* pos_intra_loss.mean()           (tuple element 0) */
    DG_OUT_LOSS_INTER = 1, /* pos_inter_loss.mean()           (element 2) */
    DG_OUT_LOSS_NEG   = 2, /* neg_inter_loss.mean()           (mean of element 4) */
    DG_OUT_LOSS_DEPTH = 3, /* depth_feat_loss.mean()          (element 6) */
    DG_OUT_CD_INTRA   = 4, /* pos_intra_cd.mean()             (mean of element 1) */
    DG_OUT_CD_INTER   = 5, /* pos_inter_cd.mean()             (mean of element 3) */
    DG_OUT_CD_NEG     = 6, /* neg_inter_cd.mean()             (mean of element 5) */
    DG_OUT_DD         = 7, /* depth_feat_cd.mean() (= mean of dd, element 7) */
    DG_OUT_TOTAL      = 8, /* w_intra*[0] + w_inter*[1] + w_neg*[2] + w_depth*[3]: the term training_step adds to its loss */
    DG_OUT_COUNT      = 9
};

int dg_version(void);
const char* dg_last_error(void);

/* Bytes of workspace dg_corr_forward/backward/materialize need for this descriptor. */
size_t dg_corr_workspace_bytes(const dg_corr_desc* desc);

/*
 * Forward of the whole loss (replaces ContrastiveCorrelationLoss.forward after the coordinate
 * draw, src/modules.py:1323-1367): sample() of feats/code at coords1, feats_pos/code_pos and the
 * n_neg negatives at coords2 (modules.py:822-825), norm() (modules.py:789-790), the
 * feature/code correlations (modules.py:797-809), pointwise centering, clamp, shift and the
 * mean reductions of helper() (modules.py:1231-1254) and of depth_feature_correlation()
 * (modules.py:1256-1278).
 *
 *  orig_feats, orig_feats_pos : fp32 (B,C,h,w) contiguous NCHW
 *  orig_code,  orig_code_pos  : fp32 (B,D,h,w), or (B,D,code_h,code_w) when the descriptor names a code-map size
 *  depth                      : fp32 (B,1,depth_h,depth_w) or NULL (required with DG_DEPTH_TERM)
 *  coords1, coords2           : fp32 (B,S,S,2) in [-1,1]  (what the reference passes to sample()); (B,S,1,2) with DG_LINE_GRID
 *  perms                      : int64 (n_neg,B) = super_perm() draws (modules.py:1184-1188,1341)
 *  out_scalars                : fp32 [DG_OUT_COUNT]
 * With DG_NEED_GRAD the unit-upstream gradient pieces are left in the workspace for
 * dg_corr_backward, which must be called with the SAME desc, coords, perms and workspace.
 */
int dg_corr_forward(const dg_corr_desc* desc,
                    const float* orig_feats, const float* orig_feats_pos,
                    const float* orig_code, const float* orig_code_pos,
                    const float* depth,
                    const float* coords1, const float* coords2, const int64_t* perms,
                    float* out_scalars,
                    void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * dg_corr_forward that also DRAWS the negatives' batch maps - the `super_perm` calls at the top of the reference's negative
 * loop (src/modules.py:1184-1188, 1340-1342) happen inside the forward there too.  perms_out (n_neg, B) is written (the same
 * values dg_super_perms with that seed / that state would write: perm_state non-NULL selects the
 * device-resident generator and advances it, else `seed`) and must be handed to dg_corr_backward / dg_corr_materialize.  On
 * the identity grid the draw rides in the first launch of the forward (no launch of its own); with general coordinates, whose
 * first launch already reads the maps, it is launched first.
 */
int dg_corr_forward_draw(const dg_corr_desc* desc,
                         const float* orig_feats, const float* orig_feats_pos,
                         const float* orig_code, const float* orig_code_pos,
                         const float* depth,
                         const float* coords1, const float* coords2, int64_t* perms_out, uint64_t seed, void* perm_state,
                         float* out_scalars,
                         void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * dg_corr_forward / dg_corr_forward_draw with the Dropout2d of the two feature maps applied INSIDE the operand preparation
 * instead of by their producer (`feats = self.dropout(image_feat)`, nn.Dropout2d, src/modules.py:122-137: the last thing
 * DinoFeaturizer.forward does to the tensor this loss receives as orig_feats / orig_feats_pos).  The caller hands in the
 * UN-dropped features and the draw:
 *  feat_keep, feat_pos_keep : fp32 (B,C) keep flags 1 / 0 of orig_feats / orig_feats_pos, either may be NULL (no dropout)
 *  keep_scale               : 1/(1-p), applied to the kept channels
 * The operands are built from x * (keep * keep_scale) - the fp32 product the producer would have stored - so every output has
 * the bits of the call on the dropped features; what is saved is that tensor's round trip through HBM (38.5 MB written and read
 * per map at the headline shape).  Identity grid only (DG_IDENTITY_GRID); DG_ERR_UNSUPPORTED otherwise.
 *  perms, draw_perms, seed, perm_state : draw_perms != 0: as perms_out / seed / perm_state of dg_corr_forward_draw; 0: perms
 *                                        is read, as by dg_corr_forward.
 * dg_corr_backward does not read the feature maps.  (version 113)
 */
int dg_corr_forward_masked(const dg_corr_desc* desc,
                           const float* orig_feats, const float* orig_feats_pos,
                           const float* orig_code, const float* orig_code_pos,
                           const float* depth,
                           const float* coords1, const float* coords2, int64_t* perms, int32_t draw_perms, uint64_t seed,
                           void* perm_state, const float* feat_keep, const float* feat_pos_keep, float keep_scale,
                           float* out_scalars,
                           void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * The forward of DepthContrastiveCorrelationLoss (src/modules.py:1370-1463; the lines that differ: :1427-1438) - dg_corr_forward
 * with ONE difference: the self-correlation (intra) pair-set takes its feature correlation fd from a second feature map,
 *  intra_feats : fp32 (B,C,h,w), the shape of orig_feats - the reference's depth_aug_feats -
 * which is sampled at coords1 and normalised exactly as orig_feats is (:1433) and is the feature operand of BOTH sides of pair-set 0
 * (pos_intra, :1437-1438) and of nothing else.  The inter pair-set and the negatives keep orig_feats / orig_feats_pos; every code
 * operand, the pointwise centering, shifts, clamp, out_scalars and DG_OUT_TOTAL are dg_corr_forward's.  (The reference also samples
 * depth_aug_feats_pos, :1434, and never reads the result: this entry does not take it.)
 * One entry for given and drawn batch maps, as dg_corr_forward_masked: draw_perms != 0: perms / seed / perm_state are perms_out / seed
 * / perm_state of dg_corr_forward_draw; 0: perms is read, as by dg_corr_forward.
 * Preparation: intra_feats is gathered by the launches that gather orig_feats (more blocks of the sampler's launch and of the
 * operand-building launch: no launch of its own) into one more prepared operand, to which the plan points pair-set 0.  Both sides of
 * the pair-set are the same operand, so its gradient is formed by symmetry as before; dg_corr_backward, dg_corr_backward_total,
 * dg_corr_cd_hist and dg_corr_materialize (cd of every pair-set, loss of the inter pair-set and the negatives - NOT the un-reduced
 * intra loss, which they would form from orig_feats) are called with the same descriptor and workspace and are unchanged: the backward
 * reads no feature map and cd depends on none.
 * Workspace: dg_corr_workspace_bytes_intra_feats(desc) bytes - the descriptor cannot tell the two entries apart, so the extra
 * operand has a query of its own; it lies behind the regions of dg_corr_workspace_bytes(desc), whose result and layout are unchanged.
 * Served: general coordinates per image on every route the plan picks for them (the fused small-grid kernel up to 160 positions,
 * the blob kernels above), C <= 768, D <= 128, n_neg <= DG_MAX_NEG - 1 (the operand tables hold DG_MAX_NEG + 2 operands, one of them
 * now the intra features), DG_NEED_GRAD on and off, every clamp / pointwise / stabalize combination.  DG_ERR_UNSUPPORTED, with the
 * reason in dg_last_error(): DG_IDENTITY_GRID, DG_SHARED_COORDS, DG_LINE_GRID, DG_DEPTH_TERM (the reference class draws random or
 * salience coordinates only and has no depth term; `depth` is not read), a code-map size other than (h, w), intra_feats == NULL.
 * No atomics; two calls give the same bits; with intra_feats == orig_feats (a copy) every output has the bits of dg_corr_forward.
 */
size_t dg_corr_workspace_bytes_intra_feats(const dg_corr_desc* desc);
int dg_corr_forward_intra_feats(const dg_corr_desc* desc,
                                const float* orig_feats, const float* orig_feats_pos,
                                const float* orig_code, const float* orig_code_pos,
                                const float* depth,
                                const float* coords1, const float* coords2, int64_t* perms, int32_t draw_perms, uint64_t seed,
                                void* perm_state, const float* intra_feats,
                                float* out_scalars,
                                void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * Backward (replaces autograd through helper()/sample(), SURVEY.md section 9 "Gradient"):
 *  grad_scalars : fp32 [DG_OUT_COUNT] device = upstream gradient of the out_scalars vector: entries 0..3 (the four
 *                 loss means) and DG_OUT_TOTAL are used, effective d/d(loss mean i) = g[i] + g[DG_OUT_TOTAL] * w_i;
 *                 the cd means carry no gradient
 *                 (DG_OUT_LOSS_INTRA..DG_OUT_LOSS_DEPTH order)
 *  grad_code, grad_code_pos : fp32, the shape of orig_code ((B,D,h,w) or (B,D,code_h,code_w)), overwritten.
 *  coords1, coords2, perms  : the SAME arrays the forward of this workspace ran on.  With general coordinates the adjoint of
 *                 sample() gathers through inverse tap records that the FORWARD built from its coords (first launch of a
 *                 DG_NEED_GRAD forward); the backward does not rebuild them, so coords that differ from the forward's are
 *                 not detected and give the gradient at the forward's sample positions.  Only valid after a forward with
 *                 DG_NEED_GRAD on this workspace, before the next forward overwrites it.
 */
int dg_corr_backward(const dg_corr_desc* desc,
                     const float* grad_scalars,
                     const float* coords1, const float* coords2, const int64_t* perms,
                     float* grad_code, float* grad_code_pos,
                     void* workspace, size_t workspace_bytes, dg_stream_t stream);
/* Same with the upstream gradient of out_scalars[DG_OUT_TOTAL] alone (a device scalar): effective d/d(loss mean i) =
 * grad_total[0] * w_i.  What `total.backward()` needs - no 9-element gradient vector has to be assembled first. */
int dg_corr_backward_total(const dg_corr_desc* desc,
                           const float* grad_total,
                           const float* coords1, const float* coords2, const int64_t* perms,
                           float* grad_code, float* grad_code_pos,
                           void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * Optional full tensors the reference returns un-reduced (src/modules.py:1352-1367), computed
 * from the operands dg_corr_forward left in the workspace.  which: 0 = pos_intra, 1 = pos_inter,
 * 2+k = negative k, -1 = depth term.  out_cd / out_loss: fp32 (B,S,S,S,S) ((B,1,S,1,S) with DG_LINE_GRID) or NULL.
 * For which == -1 out_cd receives dd (tuple element 7).
 */
int dg_corr_materialize(const dg_corr_desc* desc, int32_t which,
                        float* out_cd, float* out_loss,
                        void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * dg_corr_materialize for calls with DG_SHARED_COORDS (the dense identity grid), where the negatives' operands are the anchors'
 * operand read through their batch maps: `perms` = the (n_neg, B) maps the forward used (dg_corr_forward's argument or what
 * dg_corr_forward_draw wrote).  The reference returns these tensors on every grid (src/modules.py:1352-1367; `hist_freq` steps of
 * src/train_segmentation.py histogram them).  Without DG_SHARED_COORDS it is dg_corr_materialize (perms may be NULL).
 */
int dg_corr_materialize_shared(const dg_corr_desc* desc, int32_t which, const int64_t* perms, float* out_cd, float* out_loss,
                               void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * Histograms of the un-reduced code correlations cd of pair-sets first .. first + count - 1 (0 = pos_intra, 1 = pos_inter, 2+k =
 * negative k) - what the reference's training_step logs every cfg.hist_freq steps (src/train_segmentation.py:229-231, 298-301) -
 * WITHOUT the (B,S,S,S,S) tensors: every cd is formed again from the operands the forward left in the workspace, binned and
 * dropped.  One memset node and one launch for all requested pair-sets, on the caller's stream; no allocation, no host
 * synchronisation.  Works on every grid and in both forms of the forward's outputs.
 *  nbins, lo, hi : 1 <= nbins <= 256 uniform bins over [lo, hi], lo < hi finite.  torch.histc's rule: bin = floor((v - lo) * nbins /
 *                  (hi - lo)), v == hi in the last bin.  ONE difference: a value outside [lo, hi] is counted in the nearest end bin,
 *                  not dropped (a cosine leaves [-1, 1] by a rounding error only), so every row sums to B * P * P.
 *  out_counts    : int64 (count, nbins), overwritten.
 *  perms         : the forward's (n_neg, B) batch maps; may be NULL unless a negative of a DG_SHARED_COORDS call is asked for.
 * first < 0 is refused: the depth term's un-reduced tensor is dd, which the reference does not histogram.
 * Valid after a forward on this workspace with the same desc and perms, before the next forward; the call only READS the
 * workspace, so a later dg_corr_backward is still valid.  The values are those of the operands the forward's kernels multiply:
 * fp16 code operands on grids above 160 positions and the identity grid (|error of a cd| <= 1e-3), fp32 rows below (2e-5).
 */
int dg_corr_cd_hist(const dg_corr_desc* desc, int32_t first, int32_t count, const int64_t* perms,
                    int32_t nbins, float lo, float hi, int64_t* out_counts,
                    void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * Depth-guided sample locations (replaces farthest_point_sampling_depth, src/modules.py:999-1037,
 * with depth2points :988-996 and fps :939-985): adaptive_avg_pool2d of depth to (h,w), pinhole
 * back-projection with fov=90 (radians, quirk Q5), farthest point sampling of S*S points starting
 * at index 0, re-emitted in row-major order.
 *  depth      : fp32 (B,1,depth_h,depth_w)
 *  depth_pos  : NULL, or a second tensor like depth: the two calls of one step (src/modules.py:1304-1308: the anchors' depth, then
 *               the positives') as one launch over 2B maps - the sampler is sequential per image, so both run side by side on twice as
 *               many CUs and the caller needs no concatenated copy
 *  out_coords : fp32 (B,S,S,2), already mapped *2-1 as the caller does (modules.py:1305-1308); with depth_pos (2B,S,S,2): [0,B) from
 *               depth, [B,2B) from depth_pos
 *  out_inds   : int32 (B,S*S) - (2B,S*S) with depth_pos - selection order (may be NULL)
 *  workspace  : >= dg_fps_workspace_bytes(B,h,w) bytes, of (2B,h,w) with depth_pos (the pooled depth maps, written by a launch over
 *               the whole chip in front of the sampler)
 */
size_t dg_fps_workspace_bytes(int32_t B, int32_t h, int32_t w);
int dg_fps_coords(const float* depth, const float* depth_pos, int32_t B, int32_t depth_h, int32_t depth_w,
                  int32_t h, int32_t w, int32_t S, float* out_coords, int32_t* out_inds,
                  void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * Depth-and-feature-guided sample locations (cfg.dg_fps_feats): farthest_point_sampling_depth (src/modules.py:999-1037) with its
 * `fps(point_cloud, n*n)` call (:1020) replaced by `fps_depth_feats(point_cloud, feats, n*n)` (:1124-1180) on the feature rows the
 * reference forms at :1017 and drops - the sampler depth_sampling = 'fps_depth_feat' names and the reference never calls (quirk
 * Q13: without cfg.dg_fps_feats that mode stays dg_fps_coords).  Per round, over the points not yet selected: squared distance to
 * the last selected point in space (3 coordinates) and in feature space (C channels, direct fp32 sum of squared differences),
 * each divided by its maximum over those points, summed, folded into the running minimum; the first arg-max is selected next.
 * One deviation: where a maximum is 0 (all points left coincide with the last one in space - a zero depth map - or in feature
 * space) the reference divides 0 / 0 and selects on NaNs; here that term contributes 0.
 *  depth, depth_pos      : as dg_fps_coords
 *  feats                 : fp32 (B,C,h,w), unnormalised, as handed to the loss; feats_pos: NULL exactly when depth_pos is
 *  out_coords, out_inds  : as dg_fps_coords
 *  workspace             : >= dg_fps_feats_workspace_bytes(B,h,w) bytes, of (2B,h,w) with depth_pos; required
 * Refused before any launch: a null or misaligned pointer, the grid limits of dg_fps_coords (h*w <= 4096, depth no smaller than the
 * grid), S*S > h*w, C < 1 (and C > 16384, a pooled row's depth rows beyond 64 KB).  No atomics; two calls give equal bits.
 */
size_t dg_fps_feats_workspace_bytes(int32_t B, int32_t h, int32_t w);
int dg_fps_feats_coords(const float* depth, const float* depth_pos, const float* feats, const float* feats_pos,
                        int32_t B, int32_t C, int32_t depth_h, int32_t depth_w, int32_t h, int32_t w, int32_t S,
                        float* out_coords, int32_t* out_inds, void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * dg_fps_coords on pooled grids above its 4096 positions: 1 <= h*w <= 65536, one block per image.  Needed under cfg.use_true_labels,
 * where the loss's signal - and so the grid farthest_point_sampling_depth pools the depth to (src/modules.py:1003) - has the labels'
 * resolution (src/train_segmentation.py:219-225).  A thread keeps its points' pooled depth and running distance and rebuilds the
 * point from the depth in every round with depth2points' operations (src/modules.py:985-996) in dg_fps_coords' order; rounds, ties
 * (first arg-max) and the row-major output are dg_fps_coords': on a grid both entries accept the results are equal bit for bit.
 * dg_fps_coords itself is unchanged.
 *  depth, depth_pos, out_coords, out_inds : as dg_fps_coords
 *  workspace : >= dg_fps_large_workspace_bytes(B,h,w) bytes, of (2B,h,w) with depth_pos - the pooled depth maps; not read, and may
 *              be NULL, where the depth maps have the grid's own size (the pooling is then the identity and nothing is copied)
 * Refused before any launch: a null or misaligned pointer, h*w > 65536, depth smaller than the grid, S*S > h*w, S*S > 8192 (the
 * selection order lives in LDS), a pooled row whose depth rows exceed 64 KB of LDS, a workspace too small for the pooling.
 */
size_t dg_fps_large_workspace_bytes(int32_t B, int32_t h, int32_t w);
int dg_fps_coords_large(const float* depth, const float* depth_pos, int32_t B, int32_t depth_h, int32_t depth_w,
                        int32_t h, int32_t w, int32_t S, float* out_coords, int32_t* out_inds,
                        void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * The supervised signal of the correlation loss (cfg.use_true_labels): one_hot_feats(label + 1, n_classes + 1)
 * (src/train_segmentation.py:219-225; src/utils.py:64-65) without the int64 (B,H,W,K) tensor and its permuted copy.
 *  label     : int64 (B,H,W), values in [-1, n_classes - 1], read in place; label_pos: the same shape, or NULL
 *  out       : fp32 (B, n_classes + 1, H, W) - (2B, ...) with label_pos, rows [0,B) from label, [B,2B) from label_pos; channel
 *              label + 1 of a pixel is 1.0, every other 0.0; every element written exactly once (no atomics, no LDS)
 * A label outside the range selects no channel (an all-zero pixel); the reference's F.one_hot raises there - the caller checks.
 * Refused before the launch: a null pointer, labels not 8-byte or out not 4-byte aligned, n_classes + 1 > 256, 2B > 65535,
 * H*W > 2^24.
 */
int dg_label_onehot(const int64_t* label, const int64_t* label_pos, int32_t B, int32_t n_classes, int32_t H, int32_t W, float* out,
                    dg_stream_t stream);

/*
 * The reference's sample() (src/modules.py:822-825: F.grid_sample(t, coords.permute(0, 2, 1, 3), padding_mode='border',
 * align_corners=True), bilinear) as rows, the four taps of every (position, channel) read in place from the NCHW map: no
 * channel-last copy, no LDS.  It is the sampler dg_corr_forward runs on feature maps above 16384 and up to 65536 positions (the
 * label-size signal of cfg.use_true_labels), behind an entry of its own for maps of 1 to 65536 positions.
 *  map      : fp32 (B,K,h,w)           coords : fp32 (B,S,Sh,2), (x, y) in [-1, 1]; values outside are clamped to the border
 *  srcidx   : int64 (B) or NULL: image n is sampled from map[srcidx[n]] at coords[n] (the negatives' batch maps); an entry outside
 *             [0, B) is the caller's error and is clamped into it
 *  out      : (B, Sh*S, Kout) rows, position p = i*S + j sampled at coords[n][j][i]; fp32, or bf16 with as_bf16 != 0; channels
 *             K..Kout-1 are zero.  Every element is written exactly once (no atomics): two calls give equal bits.
 * Tap arithmetic: x = ((c + 1) / 2) * (w - 1), clamped to [0, w - 1], floor, the four weight products with the weights of taps
 * beyond the border zeroed, then a0 * w00 followed by three fused multiply-adds - the operations of every sampler of this library.
 * Refused before the launch: a null map, coords or out; map, coords or out not 4-byte, srcidx not 8-byte aligned; a non-positive
 * dimension; h*w > 65536; Kout < K or Kout % 4 != 0; B > 65535.
 */
int dg_sample_rows(const float* map, const float* coords, const int64_t* srcidx, int32_t B, int32_t K, int32_t h, int32_t w,
                   int32_t S, int32_t Sh, int32_t Kout, int32_t as_bf16, void* out, dg_stream_t stream);

/*
 * Salience-guided sample locations (replaces sample_nonzero_locations, src/modules.py:1191-1204, the cfg.use_salience
 * branch of the coordinate draw, :1290-1297): every position gets a uniformly drawn non-zero pixel of its image's
 * salience map (torch.nonzero = row-major order), returned as the reference does: both pixel coordinates divided by
 * the map HEIGHT (t.shape[1]), mapped *2-1 and flipped to (x, y).  The randomness comes from the caller as iid uniforms
 * in [0,1) (torch.rand); rank = min(int(u * count), count - 1).  An image without non-zeros gets
 * min(int(u_fallback * H), H - 1) for both coordinates (modules.py:1198).
 *  salience   : fp32 (B,H,W)         u_sel : fp32 (B,n)       u_fallback : fp32 (B,n,2)
 *  out_coords : fp32 (B,n,2); n = S*S, so the caller views it as (B,S,S,2)
 */
int dg_salience_coords(const float* salience, int32_t B, int32_t H, int32_t W, int32_t n,
                       const float* u_sel, const float* u_fallback, float* out_coords, dg_stream_t stream);

/*
 * Depth-distribution sample locations (replaces simple_depth_informed_sampling, src/modules.py:828-883, the
 * cfg.depth_sampling == 'simple' branch, :1299-1302): adaptive_max_pool2d of depth to (h,w), rounded to one decimal;
 * a depth value is drawn with probability count/h*w (the reference's multinomial over torch.unique counts), then one of
 * the pixels holding that value uniformly (torch.nonzero order).  u_value / u_pick are the caller's iid uniforms for
 * the two draws: sorted position R = min(int(u_value * h*w), h*w - 1) selects the value, min(int(u_pick * run), run - 1)
 * the pixel inside its run.
 *  depth      : fp32 (B,1,depth_h,depth_w)      u_value, u_pick : fp32 (B,n)      h*w <= 4096
 *  out_coords : fp32 (B,n,1,2) = ((row + .5) / h, (col + .5) / w) * 2 - 1 (the *2-1 of modules.py:1300 included);
 *               feed it to dg_corr_forward with DG_LINE_GRID and S = n.
 */
int dg_simple_depth_coords(const float* depth, int32_t B, int32_t depth_h, int32_t depth_w, int32_t h, int32_t w,
                           int32_t n, const float* u_value, const float* u_pick, float* out_coords, dg_stream_t stream);

/*
 * Confusion-matrix accumulation of the validation metrics (replaces the bincount of UnsupervisedMetrics.update /
 * update_cherry, src/utils.py:222-232, 279-289): stats[pred][actual] += 1 for every element with
 * 0 <= actual < n_classes and 0 <= pred < n_classes (the reference masks preds with n_classes as well, so the extra
 * clusters' rows stay zero).  Counts are exact integers: bit-identical to torch.bincount; under data parallelism the
 * matrices of the ranks are summed with one all-reduce (torchmetrics dist_reduce_fx="sum", src/utils.py:214-220).
 *  preds, target : int64 [count] (any shape, flattened)     stats : int64 (n_classes + extra_clusters, n_classes), in/out
 */
int dg_confusion_update(const int64_t* preds, const int64_t* target, int64_t count,
                        int32_t n_classes, int32_t extra_clusters, int64_t* stats, dg_stream_t stream);

/*
 * Depth propagation of the LHP branch (replaces LocalHiddenPositiveProjection.forward_depth up to its projection head,
 * src/modules.py:273-335: adaptive_avg_pool2d + depth2points(fov=90) per image, pairwise point distances, row-wise min-max
 * normalisation, map = 1 - d where d <= the row's 1 % quantile (torch.quantile, linear), out[:, p] = mean_q map[p][q] code[:, q]).
 * The (B,P,P) distance / map tensors are never formed.  Distances are the direct float32 formula; the reference's
 * torch.cdist takes its matmul path for P > 25, so outputs agree with it to about 1e-4 relative, not bit for bit.
 *  code   : fp32 (B,D,h,w), D <= 128, h*w <= 4096        depth : fp32 (B,1,depth_h,depth_w)
 *  out    : fp32 (B,D,h,w) = code_mixed
 *  points : fp32 (B,3,h*w) scratch, stats : fp32 (B,h*w,3) = per-row (min, max, quantile): both are inputs of the backward
 * dg_lhp_backward: grad_code[:, q] = (1/P) sum_p map[p][q] grad_out[:, p], with the same points / stats.
 */
int dg_lhp_forward(const float* code, const float* depth, int32_t B, int32_t D, int32_t h, int32_t w,
                   int32_t depth_h, int32_t depth_w, float* out, float* points, float* stats, dg_stream_t stream);
int dg_lhp_backward(const float* grad_out, const float* points, const float* stats, int32_t B, int32_t D, int32_t h, int32_t w,
                    float* grad_code, dg_stream_t stream);

/*
 * The other propagation maps of the LHP branch, up to the projection head.  `mode`:
 *  DG_LHP_ATTN        LocalHiddenPositiveProjection.forward_attn (src/modules.py:235-271): attn[:, :, 1:, 1:] averaged over
 *                     the heads, row-wise min-max normalised, zeroed above the row's 99 % quantile (torch.quantile, linear);
 *                     out[:, p] = mean_q map[p][q] code[:, q]
 *  DG_LHP_ORIG_DEPTH  OriginalLocalHiddenPositiveProjection.forward_depth (:436-487): map = 1 - normalised point distance,
 *                     zeroed where the distance is above the row mean, times the clipped 3x3 neighbourhood mask (:356-383);
 *                     out[:, p] = sum_q map[p][q] code[:, q] / divide_num[p]
 *  DG_LHP_ORIG_ATTN   OriginalLocalHiddenPositiveProjection.forward_attn (:403-434): heads-mean attention normalised with
 *                     the row's 10 % / 90 % quantiles, zeroed below the row mean, same mask and divisor
 * The reference leaves divide_num all zero (it is re-created inside the constructor loop and never filled, :354,382), so its
 * Original variants return sum / 0; `divide` is an input here so that both that behaviour and a repaired table can be run.
 *  code  : fp32 (B,D,h,w), D <= 128, h*w <= 4096      attn : fp32 (B,heads,h*w+1,h*w+1) (CLS row / column first)
 *  depth : fp32 (B,1,depth_h,depth_w) (ORIG_DEPTH)    divide : fp32 (h*w) (ORIG_*)
 *  out   : fp32 (B,D,h,w)
 *  map   : ATTN: fp32 (B,P,P), ORIG_*: fp32 (B,P,9): the weights, written by the forward and read by the backward
 *  points: fp32 (B,3,h*w) scratch (ORIG_DEPTH)
 * dg_lhp_map_backward: grad_code[:, q] = sum_p map[p][q] grad_out[:, p] * (1/P, or 1/divide[p]); no gradient reaches attn / depth
 * (the reference's come from a frozen backbone / the data loader).
 */
enum { DG_LHP_ATTN = 0, DG_LHP_ORIG_DEPTH = 1, DG_LHP_ORIG_ATTN = 2 };
int dg_lhp_map_forward(int32_t mode, const float* code, const float* attn, const float* depth, const float* divide,
                       int32_t B, int32_t D, int32_t h, int32_t w, int32_t heads, int32_t depth_h, int32_t depth_w,
                       float* out, float* map, float* points, dg_stream_t stream);
int dg_lhp_map_backward(int32_t mode, const float* grad_out, const float* map, const float* divide, int32_t B, int32_t D,
                        int32_t h, int32_t w, float* grad_code, dg_stream_t stream);

/*
 * The similarity slice of the offline nearest-neighbour search (replaces `pairwise_sims = torch.einsum("nf,mf->nm", batch_feats,
 * normed_feats)`, src/precompute_knns.py:106-108): out[i][j] = <queries[i], feats[j]>, fp32 products and fp32 accumulation on the
 * fp32 MFMA.
 *  queries : fp32 (rows_q, F), row stride q_stride elements      feats : fp32 (n, F), row stride f_stride      F >= 1
 *  out     : fp32 (rows_q, n), row stride out_stride
 * Any row stride >= F and any 4-byte-aligned pointer is accepted: rows are read with 16-byte loads when F is a multiple of 4 and
 * every row starts on a 16-byte boundary, with 4-byte loads otherwise - the same result bits either way.
 */
int dg_knn_similarities(const float* queries, const float* feats, int64_t rows_q, int64_t n, int32_t F, int64_t q_stride,
                        int64_t f_stride, float* out, int64_t out_stride, dg_stream_t stream);

/*
 * Row-wise top-k (replaces `torch.topk(pairwise_sims, 30)[1]` of the offline nearest-neighbour search,
 * src/precompute_knns.py:108-112; the similarity slice `einsum("nf,mf->nm")` itself is a plain GEMM and stays a library
 * call in the host mirror).  Row r of the result holds the column indices of the k largest values of row r, ordered by
 * value descending, ties by ascending column (torch.topk leaves the tie order unspecified).
 *  vals : fp32 (rows, cols) with row stride `row_stride` elements     k <= 64, k <= cols < 2^32
 *  out_idx : int64 (rows, k)        out_val : fp32 (rows, k) or NULL
 */
int dg_topk_rows(const float* vals, int64_t rows, int64_t cols, int64_t row_stride, int32_t k,
                 int64_t* out_idx, float* out_val, dg_stream_t stream);

/*
 * Negative-pair batch permutations (replaces super_perm, src/modules.py:1184-1188, called n_neg times per step at
 * :1336-1339): `count` independent uniform random permutations of 0..B-1 with fixed points bumped by one modulo B
 * (quirk Q6: B == 1 gives [0]).  Row r of the result is the argsort of row r of count*B iid uniform keys (ties by index), which is
 * a uniform random permutation like torch.randperm.  The keys come from one of three sources:
 *  keys  : fp32 (count, B) from the caller (torch.rand), or NULL
 *  state : NULL, or the generator state ON THE DEVICE = {seed, draws so far, 0} (three 64-bit words owned by the caller, zero the
 *          third): key(r, i) = Philox4x32-10({seed, draws}; counter r*B + i) >> 8 as a float in [0,1), drawn inside the launch, which
 *          advances `draws` on the device.  Nothing about the draw is baked into the launch, so a call recorded in a hipGraph
 *          (torch.cuda.graph around the training step) yields new permutations on every replay - the reference draws them with the
 *          device generator at the same place, src/modules.py:1184-1188,1336-1339.  keys and state together are refused.
 *  seed  : with neither: the same Philox draw keyed by this 64-bit value, fresh per call from the caller's own RNG - one launch per
 *          step instead of rand + sort
 *  out   : int64 (count, B)      B <= 8192; count == 0 returns DG_OK and looks at no pointer
 */
int dg_super_perms(const float* keys, uint64_t seed, uint64_t* state, int32_t count, int32_t B, int64_t* out, dg_stream_t stream);
/* The random sample coordinates of a step (`torch.rand(B, S, S, 2) * 2 - 1` for coords1 and coords2, src/modules.py:1310-1321) from
 * the same device-resident generator: n floats in [-1, 1) into `out`, one launch for both coordinate sets; advances the state.  For
 * steps recorded in a hipGraph (cfg.dg_graph_safe), where torch's generator costs two launches per tensor and two fills per replay;
 * the values are NOT torch's stream (neither are that mode's permutations).  (version 112) */
int dg_rand_coords_state(uint64_t* state, int64_t n, float* out, dg_stream_t stream);
/* Dropout2d keep flags of a graph-recorded step from the same generator: n floats, 1 with probability p_keep else 0 (what the head's
 * keep1 / keep2 / keep3 take; the reference draws them with nn.Dropout2d, src/modules.py:122-132).  One launch for all the masks of a
 * step; advances the state; not torch's stream.  (version 112) */
int dg_rand_keep_state(uint64_t* state, int64_t n, float p_keep, float* out, dg_stream_t stream);

/*
 * norm() of the reference (F.normalize(t, dim=1, eps=1e-10), src/modules.py:789-790) over ALL C channels of an NCHW map, written as
 * `nchunks` maps of `chunk_c` channels each (the last one: the rest), every one contiguous (B, c_k, h, w): the operands of
 * DG_FEATS_UNIT calls.  On the identity grid sample() is a transposition (reference quirk Q3), so normalising the map in front of it
 * is what the reference computes behind it.
 *   src (B,C,h,w) fp32; dst[k] (B, min(chunk_c, C - k chunk_c), h, w) fp32; 1 <= nchunks <= 16, chunk_c * (nchunks - 1) < C <= chunk_c * nchunks
 */
int dg_normalize_split(int32_t B, int32_t C, int32_t h, int32_t w, const float* src, int32_t nchunks, int32_t chunk_c,
                       float* const* dst, dg_stream_t stream);

/*
 * Feature maps wider than 768 channels on SAMPLED coordinates above 160 positions (the reference normalises behind sample(),
 * src/modules.py:789-790, 822-825: the norm of a sampled vector is over all of its channels).  Two calls per channel chunk:
 *   dg_sampled_sumsq: out[n][p] (+)= sum over the chunk's channels of sample(feats[srcidx ? srcidx[n] : n], coords[n])[c][p]^2
 *     feats (B,C_k,h,w) fp32 - ONE chunk, contiguous; coords (B,S,S,2) or (B,S,1,2) with line_grid; out (B,P) fp32; accumulate 0 / 1.
 *     Once per operand: orig_feats at coords1, orig_feats_pos at coords2 and - coordinates per image (no DG_SHARED_COORDS) - orig_feats
 *     through every negative's batch map at coords2 (src/modules.py:1341-1345).
 *   dg_corr_forward_extnorm: dg_corr_forward on the chunk with feat_inv = 1 / max(sqrt(sum over ALL chunks), 1e-10), (nops, B, P) fp32,
 *     operand-major (nops = 2, or 2 + n_neg without DG_SHARED_COORDS), used instead of the chunk's own norms.
 * As with DG_FEATS_UNIT the first chunk carries the recipe's shifts and depth term, the others zero shifts and none; loss means and code
 * gradients add up (dg_corr_backward* per chunk, unchanged).
 */
int dg_sampled_sumsq(int32_t B, int32_t C, int32_t h, int32_t w, int32_t S, int32_t line_grid, const float* feats,
                     const float* coords, const int64_t* srcidx, int32_t accumulate, float* out, dg_stream_t stream);
int dg_corr_forward_extnorm(const dg_corr_desc* desc, const float* orig_feats, const float* orig_feats_pos,
                            const float* orig_code, const float* orig_code_pos, const float* depth,
                            const float* coords1, const float* coords2, const int64_t* perms, const float* feat_inv,
                            float* out_scalars, void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * The segmentation head of DinoFeaturizer (replaces `cluster1(dropout(f)) + cluster2(dropout(f))` and the third
 * `dropout(f)` of src/modules.py:122-132, modules cluster1 / cluster2 of :75-88): 1x1 convolutions as bf16 MFMA products with
 * fp32 accumulation, Dropout2d and ReLU fused (a dropped channel is a zeroed weight column, 1/(1-p) scales the accumulator),
 * the fp32 features read once.
 *  feat                 : fp32 (B,C,P), P = h*w, C <= 768 and a multiple of 8
 *  feat_pos             : NULL, or the second featurizer pass of a training step (src/train_segmentation.py:303-306: `self.net(img)`,
 *                         then `self.net(img_pos)`, with the same weights), fp32 (B,C,P): the call then covers both passes as if they
 *                         were one batch of 2B images - one launch per kernel instead of two, no concatenated copy of the features.
 *                         The second pass exists exactly when feat_pos is given: keep1/2/3 and hidden are then (2B, ...), the first
 *                         pass's B rows first; B <= 2^20.  Without it code_pos and feats_out_pos must be NULL
 *  w1,b1                : cluster1[0].weight (D,C), .bias (D); D <= 128
 *  w2a,b2a,w2b,b2b      : cluster2[0] (C,C),(C) and cluster2[2] (D,C),(D); all NULL for projection_type "linear"
 *  keep1,keep2,keep3    : fp32 (B,C) 1 = keep / 0 = drop: the three Dropout2d draws in the reference's order (cluster1's
 *                         input, cluster2's input, the returned feats); NULL = no dropout for that use (eval mode)
 *  keep_scale           : 1/(1-p)
 *  code, code_pos       : fp32 (B,D,P) out, one tensor per pass
 *  feats_out(_pos)      : fp32 (B,C,P) out = feat * keep3 * keep_scale per pass, or NULL (for both passes or neither)
 *  hidden               : bf16 (B,C,P) out: cluster2's ReLU output, needed by dg_head_backward; may be NULL without one
 *  wscratch             : dg_head_weights_bytes(C, D) bytes: the forward leaves the bf16 copies of the weight matrices there
 *                         (its first launch); dg_head_backward reads them - keep the buffer until then
 */
size_t dg_head_weights_bytes(int32_t C, int32_t D);
int dg_head_forward(int32_t B, int32_t C, int32_t D, int32_t P, const float* feat, const float* feat_pos,
                    const float* w1, const float* b1, const float* w2a, const float* b2a, const float* w2b, const float* b2b,
                    const float* keep1, const float* keep2, const float* keep3, float keep_scale,
                    float* code, float* code_pos, float* feats_out, float* feats_out_pos, void* hidden, void* wscratch,
                    dg_stream_t stream);
/* Bytes of scratch dg_head_backward needs (d hidden + the split partial sums of the three weight gradients) for B images in all:
 * pass 2 B for a call with a second pass. */
size_t dg_head_workspace_bytes(int32_t B, int32_t C, int32_t D, int32_t P);
/*
 * Gradients of the six head tensors from grad_code (B,D,P) (the backbone is frozen: nothing flows into feat).  Same feat / feat_pos /
 * keep1 / keep2 / keep_scale / hidden / wscratch as the forward.  grad_* : fp32, shapes of the parameters, overwritten; pass the
 * four cluster2 ones (and hidden) as NULL for projection_type "linear".  Bit-reproducible (no floating-point atomics).
 * With feat_pos: grad_code_pos (B,D,P) is the second pass's upstream (NULL without feat_pos), the weight gradients come out summed
 * over both passes (what autograd's accumulation of two calls yields), and the workspace is dg_head_workspace_bytes(2 B, C, D, P).
 */
int dg_head_backward(int32_t B, int32_t C, int32_t D, int32_t P, const float* feat, const float* feat_pos, const float* keep1,
                     const float* keep2, float keep_scale, const void* hidden, const void* wscratch, const float* grad_code,
                     const float* grad_code_pos, float* grad_w1, float* grad_b1, float* grad_w2a, float* grad_b2a,
                     float* grad_w2b, float* grad_b2b, void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * d loss / d image_feat of the head (opt-in: the reference's DinoFeaturizer runs its backbone under no_grad, src/modules.py:96, but
 * DinoFeaturizerWithDepth feeds the head `image_depth_feat`, which its trainable depth modules produced, src/modules.py:574-597, so
 * autograd carries the gradient through cluster1 / cluster2 and their Dropout2d, :599-600, into it):
 *     grad_feat[b,k,p] = keep_scale keep1[b,k] sum_d W1[d,k] grad_code[b,d,p] + keep_scale keep2[b,k] sum_j W2a[j,k] dh[b,j,p]
 * with dh = d hidden as dg_head_backward formed it.  Call it AFTER dg_head_backward with the same B, C, D, P, keep1, keep2,
 * keep_scale, hidden, grad_code (_pos), workspace and stream: d hidden is read from that workspace, in the layout its plan chose.  bf16
 * MFMA operands (grad_code rounded on load), fp32 accumulation; every element of grad_feat is written once (no atomics:
 * bit-reproducible), a dropped channel is exact 0.
 *  w1, w2a              : the fp32 parameters (D,C), (C,C); w2a NULL for projection_type "linear" (hidden, workspace then unused)
 *  grad_code_pos        : NULL, or the second pass's upstream: the second pass exists exactly when it is given, and the call walks the
 *                         2B images of such a dg_head_backward (keep1/2/3 (2B,C); B <= 2^20).  Without it grad_feats_out_pos and
 *                         grad_feat_pos must be NULL
 *  grad_feat(_pos)      : fp32 (B,C,P) out per pass; with two passes one of them may be NULL (not both): that pass's images are then
 *                         not computed
 *  input_workspace      : dg_head_input_workspace_bytes(C, D) bytes (the transposed bf16 weight copies, written by this call)
 * The third Dropout2d draw (feats_out) takes no part while the loss reads feats under no_grad, :1232-1234.  Where it reads the
 * attached feats_out = Dropout2d(image_feat) (opt-in on top of the opt-in: under DinoFeaturizerWithDepth the reconstruction term does,
 * src/modules.py:596-598 and src/train_segmentation.py:391-398), the gradient that reached them is added in the launch's epilogue, to
 * the element about to be stored:
 *     grad_feat[b,k,p] = (the sum above) + keep_scale keep3[b,k] grad_feats_out[b,k,p]
 *  keep3                : the third Dropout2d draw's flags fp32 (B,C) - (2B,C) with two passes - or NULL (no mask: factor 1)
 *  grad_feats_out(_pos) : fp32 (B,C,P) per pass, 16-byte aligned, or NULL: nothing is added for that pass (NULL for every pass, and
 *                         keep3 NULL: the plain input gradient, the same launches and bits).  A pass with grad_feats_out must have
 *                         its grad_feat.
 * fp32 addend on the fp32 accumulator; a channel keep3 dropped adds an exact 0; still one store per element, no atomics.
 */
size_t dg_head_input_workspace_bytes(int32_t C, int32_t D);
int dg_head_backward_input(int32_t B, int32_t C, int32_t D, int32_t P, const float* w1, const float* w2a, const float* keep1,
                           const float* keep2, const float* keep3, float keep_scale, const void* hidden,
                           const float* grad_code, const float* grad_code_pos, const float* grad_feats_out,
                           const float* grad_feats_out_pos, const void* workspace, size_t workspace_bytes, float* grad_feat,
                           float* grad_feat_pos, void* input_workspace, size_t input_workspace_bytes, dg_stream_t stream);

/*
 * Measurement aid: the launch routes dg_head_backward takes for B images in all (a call with a second pass: pass 2 B) of C channels, D code
 * channels and P positions, from the plan the launches themselves follow.  Launches nothing and touches no GPU.  out[9] =
 *   [0] d hidden route     0: k_head_dh, one block per 64-position tile      1: k_head_dh2, persistent blocks, d W2b inside
 *   [1] blocks of k_head_dh2 (0 on route 0)          [2] 64-position tiles per image
 *   [3] d W2a + d W1 launch, [4] a product alone (d W1 of the linear head, d W2b on route 0)
 *                          0: k_head_wgrad           1: k_head_wgrad2 (grouped)            2: k_head_wgrad3 (one pass; [3] only)
 *   [5] splits of [3]      [6] splits of [4]         [7] partial sums of d W2b ([1] on route 1, else [6])
 *   [8] 1: d hidden and the bf16 d code are stored step-major ([image][step of 32 positions][row][32])
 * Returns DG_OK, or the code dg_head_backward returns for a shape it refuses.
 */
int dg_head_plan_describe(int32_t B, int32_t C, int32_t D, int32_t P, int32_t* out);

/*
 * ClusterLookup.forward (src/modules.py:664-675): inner = <normalize(x), normalize(clusters)>, probs = one-hot(arg-max) when
 * alpha is NaN (the reference's `alpha is None`) else softmax(alpha * inner), loss = -mean over (B,P) of sum_n probs * inner.
 *  x : fp32 (B,D,P)   clusters : fp32 (n,D), n * (D + 1) <= 16000   inner : fp32 (B,n,P) out (the backward reads it)
 *  probs, logp (= log_softmax(alpha * inner)) : fp32 (B,n,P) out or NULL     loss : fp32 [1] out
 *  scratch : fp32 [B * ceil(P/256)]
 * dg_cluster_lookup_backward: grad_clusters (n,D) and, when grad_x is not NULL, grad_x (B,D,P) for the upstream grad_loss [1]
 * (device).  scratch : fp32 [B*n*P + B*ceil(P/64)*n*D].
 */
int dg_cluster_lookup_forward(const float* x, const float* clusters, float alpha, int32_t B, int32_t D, int32_t n, int32_t P,
                              float* inner, float* probs, float* logp, float* loss, float* scratch, dg_stream_t stream);
int dg_cluster_lookup_backward(const float* x, const float* clusters, const float* inner, float alpha, const float* grad_loss,
                               int32_t B, int32_t D, int32_t n, int32_t P, float* grad_clusters, float* grad_x, float* scratch,
                               dg_stream_t stream);

/*
 * The linear probe's loss (src/train_segmentation.py:427-434): logits (B,n,h,w) resized to the label resolution with
 * F.interpolate(mode="bilinear", align_corners=False), cross entropy over the pixels with 0 <= label < n, mean.
 *  label : int64 (B,H,W)    out3 : fp32 [3] = {sum of -log p[label], labelled pixels, loss}    scratch : fp32 [2*B*H]
 * dg_probe_ce_backward: grad_logits (B,n,h,w) for the upstream grad_loss [1]; out3 as the forward wrote it.  n*w <= 2048.
 */
int dg_probe_ce_forward(const float* logits, const int64_t* label, int32_t B, int32_t n, int32_t h, int32_t w, int32_t H, int32_t W,
                        float* out3, float* scratch, dg_stream_t stream);
int dg_probe_ce_backward(const float* logits, const int64_t* label, const float* out3, const float* grad_loss, int32_t B, int32_t n,
                         int32_t h, int32_t w, int32_t H, int32_t W, float* grad_logits, dg_stream_t stream);

/*
 * The fused probe step: both probes the training step trains on the DETACHED code (src/train_segmentation.py:421-444) in one call -
 * linear_loss = cross entropy of interpolate(lin_w . code + lin_b, (H,W), bilinear, align_corners=False) over the pixels with
 * 0 <= label < n_lin (:427-434), cluster_loss = -mean over (B,P) of max_j <normalize(clusters)_j, normalize(code)> (ClusterLookup with
 * alpha None, src/modules.py:664-675) - with the gradients of lin_w, lin_b and clusters.  The code receives no gradient, so the three
 * are linear in the upstream scalars: the forward forms them for upstream gradients of 1 and keeps them in the workspace, the backward
 * multiplies by the two scalars, which it reads on the device.
 *  code : fp32 (B,D,h,w)   label : int64 (B,H,W)   lin_w : fp32 (n_lin,D)   lin_b : fp32 (n_lin) or NULL   clusters : fp32 (n_clu,D)
 *  out3 : fp32 [3] out = {linear_loss, cluster_loss, labelled pixels}; no labelled pixel: linear_loss = 0 / 0 as dg_probe_ce_forward
 *  workspace : dg_probe_step_workspace_bytes, 16-byte aligned; the backward reads what the forward of the same shape left in it
 * dg_probe_step_backward: grad_linear, grad_cluster fp32 [1] (device) -> grad_w (n_lin,D), grad_b (n_lin), grad_clusters (n_clu,D),
 * every element written.
 * Limits (DG_ERR_UNSUPPORTED with the reason, before any launch; the sizer then returns 0): D <= 128, n_lin <= 64, n_clu <= 64,
 * n_lin * w <= 4096, B*h*w <= 2^24, H*W <= 2^30; any H, W >= 1 (non-integer ratios included).  Four launches forward, one backward, on
 * the caller's stream; no floating-point atomics: two calls give the same bits.
 */
size_t dg_probe_step_workspace_bytes(int32_t B, int32_t D, int32_t n_lin, int32_t n_clu, int32_t h, int32_t w, int32_t H, int32_t W);
int dg_probe_step_forward(const float* code, const int64_t* label, const float* lin_w, const float* lin_b, const float* clusters,
                          int32_t B, int32_t D, int32_t n_lin, int32_t n_clu, int32_t h, int32_t w, int32_t H, int32_t W,
                          float* out3, void* workspace, size_t workspace_bytes, dg_stream_t stream);
int dg_probe_step_backward(const void* workspace, size_t workspace_bytes, const float* grad_linear, const float* grad_cluster,
                           int32_t B, int32_t D, int32_t n_lin, int32_t n_clu, int32_t h, int32_t w, int32_t H, int32_t W,
                           float* grad_w, float* grad_b, float* grad_clusters, dg_stream_t stream);

/*
 * The probes' predictions at label resolution and their confusion counts: validation_step (src/train_segmentation.py:471-499:
 * F.interpolate(code, label size, bilinear, align_corners=False) -> linear_probe -> argmax / cluster_probe(code, None) -> argmax ->
 * linear_metrics / cluster_metrics.update) and eval_segmentation.py:146-170 without the CRF (code = (code + code_flip.flip(3)) / 2
 * first).  Both arg-maxes commute with the resize (the tap weights sum to 1; the pixel norm of the cosine is one positive factor),
 * so the code is projected at feature resolution and only the (n + m)-row score maps are resized, per label pixel; ties go to the
 * lowest index (torch.argmax).
 *  code : fp32 (B,D,h,w)    code_flip : fp32 (B,D,h,w), the pass on the horizontally mirrored image, or NULL
 *  lin_w : fp32 (n,D), lin_b : fp32 (n) or NULL  (Conv2d(D, n, 1))    clusters : fp32 (m,D) (ClusterLookup.clusters, normalised here)
 *  label : int64 (B,H,W)
 *  stats_lin : int64 (n,n), stats_clu : int64 (m,n), each += the counts [pred][label] over the pixels with 0 <= label < n and
 *      0 <= pred < n (UnsupervisedMetrics.update, src/utils.py:222-232: rows >= n of stats_clu are never touched), or NULL
 *  preds_lin, preds_clu : int64 (n_store,H,W) out, the arg-maxes of the first n_store images, or NULL
 *  scratch : B*h*w*(n4 + m4)*4 bytes, 16-byte aligned (n4, m4: n, m rounded up to a multiple of 4)
 * Limits (DG_ERR_UNSUPPORTED beyond them): D <= 1024, n + m <= 256, w * (n4 + m4) <= 16384.  No allocation, two launches.
 */
int dg_segment_predict(const float* code, const float* code_flip, int32_t B, int32_t D, int32_t h, int32_t w,
                       const float* lin_w, const float* lin_b, int32_t n, const float* clusters, int32_t m,
                       const int64_t* label, int32_t H, int32_t W, int64_t* stats_lin, int64_t* stats_clu, int32_t n_store,
                       int64_t* preds_lin, int64_t* preds_clu, void* scratch, size_t scratch_bytes, dg_stream_t stream);

/*
 * Label-free inference.  Replaces the loop body of src/demo_segmentation.py:59-78 without its CRF - code = (code1 + code2.flip(3)) / 2,
 * F.interpolate to the image size, linear_probe / cluster_probe, argmax, astype(uint8) - for the whole batch, and the colour lookups
 * that turn a label map into a picture (src/eval_segmentation.py:170-240: label_cmap[preds], map_clusters).  The projection and the
 * resize of the score rows are those of the scored route above, so the labels are its predictions bit for bit; there is no label
 * tensor, no metric and no n_store: every image is written.  Each output may be NULL (skipped, never touched); every byte of a
 * given output is written.
 *  code .. m : as above; n <= 255 and m <= 255 (a byte holds the id, 255 is "no class")      H, W : the size of the outputs
 *  remap : DEVICE int32 (m), cluster id -> class id, the Hungarian assignment as UnsupervisedMetrics.map_clusters forms it
 *      (src/utils.py:234-246); -1 (and any entry outside [0, 254]) is stored as 255.  NULL: the raw cluster id, as the reference demo
 *  lab_lin, lab_clu : uint8 (B,H,W) out          rgb_lin, rgb_clu : uint8 (B,H,W,3) out, interleaved
 *      per channel (alpha256 * cmap[label] + (256 - alpha256) * pix + 128) >> 8 in integers, 0 <= alpha256 <= 256;
 *      pix = clamp(rint((img * std + mean) * 255), 0, 255) (UnNormalize, src/utils.py:132-136, then the byte scale)
 *  img : fp32 (B,3,H,W) normalised; mean, std : HOST float[3].  All three may be NULL when alpha256 == 256 or no colour is asked for
 *  cmap : DEVICE uint8 (cmap_rows,3), 1 <= cmap_rows <= 256; a label >= cmap_rows - 255 among them - paints the last row
 *  scratch : B*h*w*(n4 + m4)*4 bytes, 16-byte aligned
 * Limits as above, and W <= 8176.  No allocation, no atomics, two launches; two identical calls give identical bytes.
 */
int dg_segment_labels(const float* code, const float* code_flip, int32_t B, int32_t D, int32_t h, int32_t w, const float* lin_w,
                      const float* lin_b, int32_t n, const float* clusters, int32_t m, int32_t H, int32_t W, const int32_t* remap,
                      const float* img, const float* mean, const float* std, const uint8_t* cmap, int32_t cmap_rows, int32_t alpha256,
                      uint8_t* lab_lin, uint8_t* lab_clu, uint8_t* rgb_lin, uint8_t* rgb_clu, void* scratch, size_t scratch_bytes,
                      dg_stream_t stream);
/* The same remap and paint on the predictions of the dense CRF declared below (the CRF route of src/demo_segmentation.py:71-78 and the
 * pictures of src/eval_segmentation.py:170-240).  preds : int64 (n_groups,B,H,W); preds[0] is the linear probe's map, preds[1] the
 * cluster probe's (needed only for lab_clu / rgb_clu); a value outside [0, 254] is stored as 255.  m : the length of remap.
 * The other arguments and the outputs as above.  One launch. */
int dg_label_paint(const int64_t* preds, int32_t n_groups, int32_t B, int32_t H, int32_t W, int32_t m, const int32_t* remap,
                   const float* img, const float* mean, const float* std, const uint8_t* cmap, int32_t cmap_rows, int32_t alpha256,
                   uint8_t* lab_lin, uint8_t* lab_clu, uint8_t* rgb_lin, uint8_t* rgb_clu, dg_stream_t stream);

/*
 * Dense-CRF refinement of the evaluation: src/crf.py dense_crf (pydensecrf's DenseCRF2D with addPairwiseGaussian(sxy=POS_XY_STD,
 * compat=POS_W), addPairwiseBilateral(sxy=Bi_XY_STD, srgb=Bi_RGB_STD, rgbim=image, compat=Bi_W), inference(MAX_ITER)), run per image
 * by batched_crf (src/eval_segmentation.py:55-60) on both probes' outputs (:162-167).  Mean field over permutohedral lattices built on
 * the GPU; channels come in groups (one softmax each), so several probes share one lattice and one filter pass.  Deterministic: two
 * identical calls give identical bits.
 *  img : fp32 (B,3,H,W) normalised as the loader does (T.Normalize, src/utils.py:139); the colour image is UnNormalize
 *      (src/utils.py:132-136: v * std + mean, two fp32 roundings) then mul(255).byte() (to_pil_image), BGR order; values outside
 *      [0, 255] are clamped (undefined in the reference)
 *  group_ends : HOST int32 (n_groups), strictly rising from above 0; group g = channels [ends[g-1], ends[g]); n_groups <= 8
 *  Kp : the channels with each group rounded up to a multiple of 4; Kp <= 256
 *  workspace : 256-byte aligned; the images are processed in chunks of the largest count c <= B with
 *      dg_crf_workspace_bytes(c, H, W, Kp, lattices) <= workspace_bytes (at least one image must fit: DG_ERR_WORKSPACE)
 *  The packed vertex keys must fit 63 bits (the range follows from H, W and the standard deviations; the bits above hold the image
 *  of the chunk): DG_ERR_UNSUPPORTED otherwise.
 */
/* lattices: 1 the Gaussian one (dg_crf_filter with bilateral = 0), 2 the bilateral one (bilateral = 1), 3 both (dg_dense_crf).
 * 0 on bad arguments, and where (d + 1) * chunk * H * W * Kp / 4 reaches 2^30 (d = 5 when the bilateral lattice is in). */
size_t dg_crf_workspace_bytes(int32_t chunk, int32_t H, int32_t W, int32_t Kp, int32_t lattices);
/* U = -log(clip(softmax(interp(logits)), 1e-5, 1)) per group (src/crf.py:27-35: F.interpolate(bilinear, align_corners=False) to
 * (H,W), F.softmax over the channels, pydensecrf.utils.unary_from_softmax).  logits : fp32 (B,C,h,w); unary : fp32 (B,C,H,W) out */
int dg_crf_unary(const float* logits, int32_t B, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, const int32_t* group_ends,
                 int32_t n_groups, float* unary, dg_stream_t stream);
/* The evaluation's unary straight from the code (src/eval_segmentation.py:150-167): code = (code + code_flip.flip(3)) / 2 when
 * code_flip is given, F.interpolate to (H,W), linear probe -> channels [0, n), ClusterLookup(alpha) -> channels [n, n + m), and U of
 * dg_crf_unary with the groups {n, n + m} (the softmax of the reference's log_softmax is the softmax).  The probes are projected at
 * feature resolution (dg_segment_predict's projection) and resized per label pixel; the cluster rows are divided by the norm of the
 * resized code at that pixel.  Arguments as dg_segment_predict; unary : fp32 (B, n + m, H, W) out;
 * scratch : B*h*w*(n4 + m4)*4 bytes, 16-byte aligned. */
int dg_segment_unary(const float* code, const float* code_flip, int32_t B, int32_t D, int32_t h, int32_t w, const float* lin_w,
                     const float* lin_b, int32_t n, const float* clusters, int32_t m, int32_t H, int32_t W, float alpha, float* unary,
                     void* scratch, size_t scratch_bytes, dg_stream_t stream);
/* One normalised message K~(v) = norm . K(norm . v) of a DenseKernel with NORMALIZE_SYMMETRIC (densecrf's DenseKernel::apply): the
 * Gaussian kernel over (x, y) / sxy (bilateral = 0, img may be NULL) or the bilateral one over ((x, y) / sxy, (B, G, R) / srgb).
 * Without the Potts weight.  values, out : fp32 (B,C,H,W); Kp = C rounded up to 4 for the workspace. */
int dg_crf_filter(const float* img, const float* values, int32_t B, int32_t C, int32_t H, int32_t W, int32_t bilateral, float sxy,
                  float srgb, float* out, void* workspace, size_t workspace_bytes, dg_stream_t stream);
/* Mean-field inference (densecrf's DenseCRF::inference): Q0 = softmax(-U), then n_iter times
 * Q = softmax(-U + pos_w K~g(Q) + bi_w K~b(Q)) per group (the per-pixel maximum subtracted first).
 *  unary : fp32 (B,C,H,W), C = group_ends[n_groups - 1]
 *  q : fp32 (B,C,H,W) out, or NULL    preds : int64 (n_groups,B,H,W) out, the arg-max of Q within each group (lowest index on
 *  ties; the index counts from the group's first channel), or NULL; not both NULL.  No host synchronisation, no allocation. */
int dg_dense_crf(const float* img, const float* unary, int32_t B, int32_t H, int32_t W, const int32_t* group_ends, int32_t n_groups,
                 int32_t n_iter, float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, float* q, int64_t* preds,
                 void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * The contrastive CRF loss term of the training step (cfg.crf_weight).  Replaces ContrastiveCRFLoss.forward (src/modules.py:1510-1542)
 * TOGETHER WITH its caller's resize(img, size), norm(resize(code, size)) and .mean() (src/train_segmentation.py:413-419; resize:
 * src/utils.py:60-61, bilinear, align_corners=False, no antialiasing; norm: src/modules.py:789-790, F.normalize(dim=1, eps=1e-10)):
 *      loss = mean over (B, n, n) of -sims * K,     sims_ac = S_a . S_c,
 *      K_ac = w1 exp(-|p_a - p_c|^2 / (2 alpha) - |g_a - g_c|^2 / (2 beta)) + w2 exp(-|p_a - p_c|^2 / (2 gamma)) - shift
 * with S_a the normalised resized code vector and g_a the resized image colours at sample a, p_a = (y, x) its coordinates on the
 * size x size grid.  The two maps are resized AT the n sampled positions only; neither a size x size map, nor the (B,3,n,n) guidance
 * differences, nor any (B,n,n) tensor is written: K is symmetric, so with G_a = sum_c K_ac S_c the loss is -(1 / (B n^2)) sum S_a . G_a
 * and d loss / d S_a = -(2 / (B n^2)) G_a.
 *  code      : fp32 (B,D,h,w)              img : fp32 (B,3,H,W)        (the four sizes are free: up- and down-scaling)
 *  coords    : int32 (2,n) - row 0 the y, row 1 the x of every sample on the size x size grid, shared by the batch, as the
 *              reference's torch.cat([randint(0, h), randint(0, w)]) (:1529-1531).  Device data: values outside [0, size) are
 *              clamped into it by the kernels.
 *  workspace : dg_crfloss_workspace_bytes(B, D, n) bytes (0: bad arguments), 16-byte aligned.  Sections, each starting at the next
 *              multiple of 256 bytes, Dp = D rounded up to 4:  S fp32 (B,n,Dp) | G fp32 (B,n,Dp) | g fp32 (B,n,4) | |x| fp32 (B,n)
 *              (the norm in front of the eps clamp) | q fp64 (B,n) | the blocks' fp64 partial sums.  G_a is the sum over c != a
 *              of K_ac S_c and q_a = S_a . G_a / |S_a|^2: the backward projects G_a off S_a, which removes the row's own term
 *              K_aa S_a whatever its size, so that term (K_aa = w1 + w2 - shift, the largest by far where K is nearly diagonal)
 *              enters the loss as the number it is and never the gradient.  On a row under the eps clamp (|x| < eps) G_a includes
 *              it and q_a is 0.  The stored S_a is the fp64-normalised vector rounded to fp32; what its norm still differs from 1
 *              by is taken out of the loss to first order.
 *  out_loss  : one fp32 in device memory.
 * dg_crfloss_backward: d loss / d code for the forward whose results are in `workspace` (same coords, B, D, h, w, size, n), times the
 * upstream gradient *grad_out, read on the device (no host synchronisation): through norm (dx = (g - S (S . g)) / |x| where
 * |x| >= eps, g / eps otherwise) and the resize's taps.  grad_code fp32 (B,D,h,w) is written completely, zeros included; no
 * gradient goes to img.  Destination-major, no atomics: both calls give the same bits on the same inputs.
 * Refused before any launch (DG_ERR_INVALID / DG_ERR_UNSUPPORTED): null or misaligned pointers (4 bytes; the workspace 16), D outside
 * 1..128, n outside 1..4096, size outside 1..256, non-positive B, h, w, H, W (B <= 65535, sides <= 16384), alpha, beta or gamma <= 0,
 * a workspace that is too small (DG_ERR_WORKSPACE).  fp32 arithmetic with expf and IEEE divisions; the loss sum in fp64.
 */
size_t dg_crfloss_workspace_bytes(int32_t B, int32_t D, int32_t n);
int dg_crfloss_forward(const float* code, const float* img, int32_t B, int32_t D, int32_t h, int32_t w, int32_t H, int32_t W,
                       int32_t size, const int32_t* coords, int32_t n, float alpha, float beta, float gamma, float w1, float w2,
                       float shift, void* workspace, size_t workspace_bytes, float* out_loss, dg_stream_t stream);
int dg_crfloss_backward(const void* workspace, size_t workspace_bytes, const int32_t* coords, int32_t B, int32_t D, int32_t h,
                        int32_t w, int32_t size, int32_t n, const float* grad_out, float* grad_code, dg_stream_t stream);

/*
 * The augmentation-alignment loss term of the training step (cfg.aug_alignment_weight).  Replaces the chain of
 * src/train_segmentation.py:400-411 behind `orig_code_aug`: the resize of the coordinate map (src/utils.py:60-61, bilinear,
 * align_corners=False), the two permutes, sample() (src/modules.py:822-825: grid_sample, border, align_corners=True), the two norm()
 * (src/modules.py:789-790, F.normalize(dim=1, eps=1e-10)), the einsum and the mean:
 *      ds   = resize(coord_aug.permute(0,3,1,2), n).permute(0,2,3,1)
 *      u    = sample(code, ds)               u[b,:,i,j] reads code at x = ds[b,j,i,0], y = ds[b,j,i,1] (both transpositions as written)
 *      loss = -mean over (b,i,j) of s,       s = <u / max(|u|, eps), v / max(|v|, eps)>,  v = code_aug[b,:,i,j]
 *  code      : fp32 (B,D,h,w)     code_aug : fp32 (B,D,n,n)     coord_aug : fp32 (B,H,W,2) in [-1, 1] (device data: whatever lies
 *              outside is clamped onto the border of the code map, as grid_sample's border mode does); all sizes are free.
 *  workspace : dg_augalign_workspace_bytes(B, D, h, w, n) bytes (0: bad or unsupported arguments), 16-byte aligned.  Sections, each
 *              starting at the next multiple of 256 bytes; the forward writes the first five and the last, the backward the other two:
 *              ds fp32 (B,n,n,2) | |u| fp32 (B,n^2) | |v| fp32 (B,n^2) (the norms in front of the eps clamp) | s fp32 (B,n^2) |
 *              the blocks' fp64 partial sums | d u fp32 (B,D,n^2) | B inverse tap records of ds on the code map | ds fp64 (B,n^2,2)
 *              by position (the forward writes it too).  The coordinate resize, the pixel positions and the tap weights are formed
 *              in fp64 from the fp32 inputs - the coordinates' rounding is otherwise the largest error of the term - and the weights
 *              rounded to fp32; the fp32 ds only decides which pixels list a position in the records.
 *  out_loss  : one fp32 in device memory (fp64 sum in a fixed order: the same bits on every call).
 * dg_augalign_backward: both gradients for the forward whose results are in `workspace` (same code, code_aug and sizes), times the
 * upstream gradient *grad_out, read on the device.  With c = -*grad_out / (B n^2):
 *      d v = c (u^ - s v^) / |v|,    d u = c (v^ - s u^) / |u|     where the norm is >= eps;
 *      d v = c u^ / eps,             d u = c v^ / eps              where it is below: F.normalize divides by clamp_min(|x|, eps),
 *                                                                  which under autograd is the constant eps there (x^ = x / eps)
 * and d code is the adjoint of sample() applied to d u, as a gather through position-sorted inverse tap records.  grad_code fp32
 * (B,D,h,w) and grad_code_aug fp32 (B,D,n,n) are written completely, zeros included; nothing goes to coord_aug.  No floating-point
 * atomics: two calls give the same bits.  No host synchronisation, no allocation: both calls can be captured into a graph.
 * Refused before any launch (DG_ERR_INVALID / DG_ERR_UNSUPPORTED): null or misaligned pointers (4 bytes; the workspace 16),
 * non-positive sizes, B above 65535, H or W above 16384, n above 255 (the records index the n^2 positions with 16 bits) or
 * 8 h w + 24 n^2 + 4 above 163776 (the records are built in one workgroup's LDS; 56 x 56 positions on a 56 x 56 map take 100356), a
 * workspace that is too small (DG_ERR_WORKSPACE).  fp32 arithmetic behind the tap weights, any D >= 1.
 */
size_t dg_augalign_workspace_bytes(int32_t B, int32_t D, int32_t h, int32_t w, int32_t n);
int dg_augalign_forward(const float* code, const float* code_aug, const float* coord_aug, int32_t B, int32_t D, int32_t h, int32_t w,
                        int32_t n, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* out_loss, dg_stream_t stream);
int dg_augalign_backward(const float* code, const float* code_aug, void* workspace, size_t workspace_bytes, int32_t B, int32_t D,
                         int32_t h, int32_t w, int32_t n, const float* grad_out, float* grad_code, float* grad_code_aug,
                         dg_stream_t stream);

/*
 * The reconstruction loss term of the training step (src/train_segmentation.py:391-398 under cfg.rec_weight; its decoder is the
 * nn.Conv2d(dim, n_feats, (1, 1)) of :115, stepped by net_optim when the term is on, :540-541):
 *      rec_feats = decoder(code)                                                 (:392)
 *      loss = -(norm(rec_feats) * norm(feats)).sum(1).mean()                     (:393; norm = F.normalize(dim=1, eps=1e-10), src/modules.py:789-790)
 * fused: neither rec_feats, a normalised map, their product nor a gradient of that size is written.  Per position p, with
 * y = W c_p + bias, f = feats at p, N = B h w and the upstream gradient G:
 *      ny = max(|y|, eps), nf = max(|f|, eps), s = <y, f> / (ny nf), loss = -(1/N) sum s
 *      dy = a f + b y, a = -(G/N) / (ny nf), b = (G/N) s / ny^2 where |y| > eps and 0 below (what F.normalize gives under autograd)
 *      d code_p = W^T dy, d weight = sum_p dy c_p^T, d bias = sum_p dy;  feats receives no gradient (the frozen backbone's output)
 *      except through dg_rec_feats_backward (below): d f = a y + b' f, b' = (G/N) s / nf^2 where |f| > eps and 0 below
 *  code : fp32 (B, D, h, w);  feats : fp32 (B, C, h, w);  weight : fp32 (C, D);  bias : fp32 (C);  all contiguous, 4-byte aligned
 *  keep, scale : NULL, or the Dropout2d keep flags fp32 (B, C), 1 / 0, of feats that have not been dropped yet: the kernels read
 *                feats[b,c] * (keep[b,c] != 0 ? scale : 0) - the bits of the dropped tensor (src/modules.py:122-137); scale > 0
 *  B, D, C, h, w >= 1;  D <= 128;  B C h w, B D h w and C D + C below 2^31 (DG_ERR_UNSUPPORTED otherwise, before any launch)
 *  workspace : dg_recloss_workspace_bytes(B, D, C, h, w) bytes (0 on bad arguments), 16-byte aligned.  Sections at multiples of
 *              256 bytes, in this order: |y| fp32 (B,h,w), |f| fp32 (B,h,w) - both in front of the eps clamp - s fp32 (B,h,w), one fp64
 *              sum of -s per tile of 64 positions, then the backward's partial sums of d weight (S, C, D) and d bias (S, C) fp32
 *  forward  : writes out_loss (one fp32) and the first four sections
 *  backward : same tensors and workspace as the forward; grad_out one fp32 in device memory; writes EVERY element of grad_code
 *             (B, D, h, w), grad_weight (C, D) and grad_bias (C)
 * y, dy and the three products are fp32 (fp32 MFMA: fp32 operands, fp32 accumulation); the forward's sums of |y|^2, |f|^2 and <y, f>
 * over the channels run in fp64, and s is formed from them in fp64; the loss and the partial sums of d weight / d bias (fp32 per
 * split) are combined in fp64, in launches of their own and in one fixed order.  No atomics: two calls give the same bits.  No host synchronisation.
 */
size_t dg_recloss_workspace_bytes(int32_t B, int32_t D, int32_t C, int32_t h, int32_t w);
int dg_recloss_forward(const float* code, const float* feats, const float* weight, const float* bias, const float* keep, float scale,
                       int32_t B, int32_t D, int32_t C, int32_t h, int32_t w, void* workspace, size_t workspace_bytes, float* out_loss,
                       dg_stream_t stream);
int dg_recloss_backward(const float* code, const float* feats, const float* weight, const float* bias, const float* keep, float scale,
                        void* workspace, size_t workspace_bytes, int32_t B, int32_t D, int32_t C, int32_t h, int32_t w,
                        const float* grad_out, float* grad_code, float* grad_weight, float* grad_bias, dg_stream_t stream);

/*
 * The reconstruction term's backward WITH d loss / d feats (opt-in: under DinoFeaturizerWithDepth feats = dropout(image_depth_feat)
 * is attached to the trained depth modules, src/modules.py:596-598, and the term trains them through it).  One entry that produces
 * everything in one call - call it INSTEAD of dg_recloss_backward, with the same arguments, workspace and stream:
 *  grad_feats : fp32 (B, C, h, w) out, every element written once: (a y + b' f) (keep[b,c] != 0 ? scale : 0) - the gradient of the
 *               tensor the `feats` pointer names (the un-dropped maps when keep is given; a dropped channel is an exact 0)
 *  grad_code, grad_weight, grad_bias : as dg_recloss_backward - the same bits - or all three NULL: d feats alone, from one launch
 *               that skips the W^T dy product
 * The kernel that forms d code holds y, f and the factors of every (channel, position) it visits and stores d f from those registers:
 * no further product, no atomics, two calls give the same bits.  (Named dg_rec_feats_* so that the dg_recloss_* group stays the
 * three entries it was.)
 */
int dg_rec_feats_backward(const float* code, const float* feats, const float* weight, const float* bias, const float* keep, float scale,
                          void* workspace, size_t workspace_bytes, int32_t B, int32_t D, int32_t C, int32_t h, int32_t w,
                          const float* grad_out, float* grad_code, float* grad_weight, float* grad_bias, float* grad_feats,
                          dg_stream_t stream);

/*
 * The optimisation step's Adams (src/train_segmentation.py:447-455: net_optim.step(), cluster_probe_optim.step(),
 * linear_probe_optim.step(); :537-547: three torch.optim.Adam with default betas / eps, weight_decay = 0, amsgrad = False) as ONE
 * launch over a table of segments (one per tensor); fp32 throughout:
 *      exp_avg    = exp_avg + (1 - beta1) * (grad - exp_avg)
 *      exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * grad * grad
 *      param      = param - (lr / (1 - beta1^t)) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)
 * The two tables are HOST memory, copied into the kernel's arguments (gradient pointers change every eager step; nothing is copied
 * to the device).  Tables longer than 16 segments are stepped by further launches of 16; at most 16 groups per call.
 *  device_steps = 0 : t = seg.step_host (the count AFTER this step, >= 1); both corrections are formed on the host in double.
 *  device_steps = 1 : t = *seg.step_dev + 1 (a float32 in device memory, one per segment, not shared between segments); the kernel
 *                     forms both corrections from it and stores t back, so a launch recorded into a hipGraph advances at every
 *                     replay.  tickets : uint32 [n_seg] in device memory, zero before the first call and left zero by every call
 *                     (segment k of more than 1024 elements counts its blocks in tickets[k]); may be NULL when no segment is
 *                     that long.
 * A segment with grad == NULL is skipped: parameter, moments and t untouched (torch skips parameters whose .grad is None - with
 * correspondence_weight = 0 the head receives no gradient at all).  No workspace, no host synchronisation.
 */
typedef struct dg_adam_seg {
    float* param;
    const float* grad;       /* NULL: skip the segment */
    float* exp_avg;
    float* exp_avg_sq;
    float* step_dev;         /* device_steps = 1 only */
    int64_t numel;           /* 1 .. 2^31 - 1 */
    double step_host;        /* device_steps = 0 only */
    int32_t group;           /* index into groups */
    int32_t reserved;
} dg_adam_seg;
typedef struct dg_adam_group {
    double lr, beta1, beta2, eps;
} dg_adam_group;
int dg_adam_step(const dg_adam_seg* segs, int32_t n_seg, const dg_adam_group* groups, int32_t n_groups, int32_t device_steps,
                 void* tickets, dg_stream_t stream);

/*
 * Attention forward of the frozen DINO ViT (src/dino/vision_transformer.py:80-92: attn = softmax(q @ k^T * scale), x = attn @ v,
 * transposed back to (B, N, C)) as one fused kernel: the (B, heads, N, N) matrix is never written.  Forward only (the backbone is
 * frozen, src/modules.py:34-35).
 *  qkv : fp32 (B, N, 3, heads, 64) contiguous - the output of the block's qkv linear as it stands (:82 before the permute)
 *  out : fp32 (B, N, heads * 64), the input of the block's proj linear (:89-90)
 *  head_dim : 64 only (every DINO ViT; :262-280) - DG_ERR_UNSUPPORTED otherwise, before any launch;  N >= 1, B * heads <= 65535
 *  scale : the factor on the scores (:73, head_dim ** -0.5 unless qk_scale is given)
 *  workspace : dg_attention_workspace_bytes(B, heads, N) bytes, 16-byte aligned: K and V as bf16 in MFMA fragment order
 * Arithmetic: q, k, v rounded to bf16 (nearest even), products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, scores, running
 * maximum, exponentials and row sums in fp32, the probabilities rounded to bf16 for the second product.  qkv and out must be
 * 16-byte aligned too (DG_ERR_INVALID otherwise).  Nothing outside the two tensors is read or written.
 */
size_t dg_attention_workspace_bytes(int32_t B, int32_t heads, int32_t N);      /* 0 on bad arguments */
int dg_attention_forward(const float* qkv, int32_t B, int32_t N, int32_t heads, int32_t head_dim, float scale, float* out,
                         void* workspace, size_t workspace_bytes, dg_stream_t stream);

/*
 * Linear layers of the frozen DINO ViT with their surroundings fused (src/dino/vision_transformer.py:49-65 the MLP, 68-92 qkv and
 * proj, 95-115 the block's norms and residual adds):   y = epilogue(prologue(x) W^T + b).  Forward only (the backbone is frozen).
 *  dg_vit_linear_pack : weight fp32 (Nout, K) as nn.Linear stores it -> `packed`, dg_vit_linear_packed_bytes(K, Nout) bytes: the
 *      weight rounded to bf16 (nearest even) in MFMA fragment order.  Once per weight; again only when the weight changes.
 *  dg_vit_linear_forward :
 *      x        (M, K) row-major contiguous: fp32, or bf16 with DG_LIN_IN_BF16 (the fc1 -> fc2 hand-over)
 *      gamma, beta, eps : with DG_LIN_LAYERNORM the row is normalised first (norm1 -> qkv, norm2 -> fc1; :101-104): mean and biased
 *                 variance in fp32 over the fp32 row (two passes), (x - mean) * rstd * gamma + beta in fp32.  K <= 768, fp32 x only
 *      packed   the output of dg_vit_linear_pack for this (K, Nout)
 *      bias     (Nout) fp32 or NULL
 *      DG_LIN_GELU : exact (erf) GELU in fp32 on accumulator + bias (:56, nn.GELU's default)
 *      residual (M, Nout) fp32 or NULL: out = residual + (acc + bias) in fp32 (:105-106); `out` may alias `residual`, not `x`
 *      out      (M, Nout): fp32, or bf16 with DG_LIN_OUT_BF16 (no residual then)
 *  Shapes: M >= 1 (the row tail is handled in the kernel; nothing outside the tensors is read or written); K and Nout multiples of
 *  64 up to 3072 - DG_ERR_UNSUPPORTED otherwise, before any launch.  Every pointer 16-byte aligned (DG_ERR_INVALID otherwise).
 *  Arithmetic: the A operand (LayerNorm output, or x) and W rounded to bf16, products on v_mfma_f32_32x32x16_bf16 with fp32
 *  accumulation, bias / GELU / residual in fp32.  No host synchronisation, no workspace beyond `packed`, one launch on `stream`.
 */
#define DG_LIN_LAYERNORM 1
#define DG_LIN_GELU      2
#define DG_LIN_IN_BF16   4
#define DG_LIN_OUT_BF16  8
size_t dg_vit_linear_packed_bytes(int32_t K, int32_t Nout);                     /* 0 on bad arguments */
int dg_vit_linear_pack(const float* weight, int32_t K, int32_t Nout, void* packed, dg_stream_t stream);
int dg_vit_linear_forward(const void* x, const float* gamma, const float* beta, float eps, const void* packed, const float* bias,
                          const float* residual, void* out, int32_t M, int32_t K, int32_t Nout, int32_t flags, dg_stream_t stream);

/*
 * The three-stage depth encoder of DinoFeaturizerWithDepth as fused kernels, forward and backward (src/modules.py:497-506: the
 * `depth_downscaling` stack for n_feats == 384; :557 its call; :562-563 the "sum" guidance's add; :619-631 LayerNorm2d):
 *      Conv2d(1,64,2,2), LayerNorm2d(64), GELU, Conv2d(64,128,2,2), LayerNorm2d(128), GELU, Conv2d(128,C,2,2)      [+ residual]
 * Each output position depends on one 8 x 8 depth patch, so no activation map of stage 1 or 2 is written by the forward, and the
 * backward re-forms them from the depth map.
 *  depth : fp32 (B, depth_h, depth_w) contiguous with depth_h = 8 h, depth_w = 8 w (DG_ERR_INVALID otherwise)
 *  w1 (64,1,2,2), b1 (64), gamma1, beta1 (64), w2 (128,64,2,2), b2 (128), gamma2, beta2 (128), w3 (C,128,2,2), b3 (C): the fp32
 *          parameters as nn.Conv2d / LayerNorm2d store them, contiguous
 *  residual : NULL, or fp32 (B, C, residual_h, residual_w) added in the forward's epilogue, out = residual + (acc + b3); its grid
 *          must be h x w (DG_ERR_INVALID otherwise).  It receives no gradient here: d out passes to it unchanged.
 *  C : a multiple of 64 up to 768 (DG_ERR_UNSUPPORTED otherwise);  B, h, w >= 1, B h w <= 2^24
 *  workspace : dg_depthenc_workspace_bytes(B, C, h, w, backward) bytes (0 on bad arguments), 16-byte aligned; every tensor 4-byte
 *          aligned.  Sections at multiples of 256 bytes: bf16 MFMA-fragment images of W2 and W3, made by every call (the weights
 *          change every step) - that is all the forward uses (backward = 0); with backward = 1 also the images of W2^T and W3^T, the
 *          stage-2 activation and its gradient as bf16, 2 x (tiles of 32 positions) x 512 x 32, and the fp32 partial sums of the
 *          weight gradients: 832 per block of the activation kernel (at most 512), 128 x 256 per split of d W2 (at most 64),
 *          C x 512 + 2 C per split of d W3 (at most 32).  Nothing of stage-1 size (B h w x 1024) is stored.
 *  forward  : writes EVERY element of out (B, C, h, w)
 *  backward : grad_out fp32 (B, C, h, w) contiguous; writes EVERY element of the ten gradients, shaped as their parameters.  There
 *          is no gradient for the depth map.  Needs nothing of the forward's workspace.
 * Arithmetic: stage 1 (K = 4) fp32 on the VALU; stages 2 and 3 and the backward's four products on v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation - W2, W3, the stage-1 and stage-2 activations, grad_out and the stage-2 pre-norm gradient are rounded to bf16
 * (nearest even) as MFMA operands.  LayerNorm statistics (biased variance, eps = 1e-6 inside the root), normalisation, exact (erf)
 * GELU and the biases are fp32; d b3 sums the fp32 grad_out in fp64; all partials are combined in fp64 in one fixed order.  No
 * atomics: two calls give the same bits.  No host synchronisation.
 */
size_t dg_depthenc_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t backward);
int dg_depthenc_forward(const float* depth, const float* w1, const float* b1, const float* gamma1, const float* beta1,
                        const float* w2, const float* b2, const float* gamma2, const float* beta2, const float* w3, const float* b3,
                        const float* residual, int32_t residual_h, int32_t residual_w, int32_t B, int32_t C, int32_t h, int32_t w,
                        int32_t depth_h, int32_t depth_w, float* out, void* workspace, size_t workspace_bytes, dg_stream_t stream);
int dg_depthenc_backward(const float* depth, const float* w1, const float* b1, const float* gamma1, const float* beta1,
                         const float* w2, const float* b2, const float* gamma2, const float* beta2, const float* w3, const float* b3,
                         const float* grad_out, int32_t B, int32_t C, int32_t h, int32_t w, int32_t depth_h, int32_t depth_w,
                         float* grad_w1, float* grad_b1, float* grad_gamma1, float* grad_beta1, float* grad_w2, float* grad_b2,
                         float* grad_gamma2, float* grad_beta2, float* grad_w3, float* grad_b3, void* workspace,
                         size_t workspace_bytes, dg_stream_t stream);

/*
 * Cross-attention of the depth guidance (src/modules.py:524 `cross_attn = nn.MultiheadAttention(n_feats, 8, dropout=0.1)`, :566-585)
 * between the three input projections and out_proj, forward and backward, as fused kernels: per (batch, head)
 *      O = dropout_p(softmax(q k^T * scale)) v
 * with online softmax; the (B, heads, Nq, Nk) matrix is never written, by the forward or by the backward.
 *  q : fp32 (B, Nq, heads * 48);  k, v : fp32 (B, Nk, heads * 48);  out, grad_out, grad_q as q;  grad_k, grad_v as k - all contiguous,
 *      batch-first, 16-byte aligned (DG_ERR_INVALID otherwise)
 *  head_dim : 48 only - DG_ERR_UNSUPPORTED otherwise, before any launch;  heads, Nq, Nk >= 1 (up to 2^24), B * heads <= 65535
 *  p : the dropout probability in [0, 1) (DG_ERR_INVALID otherwise); a kept probability is scaled by 1 / (1 - p).  p = 0 launches
 *      kernels without generator code.  Element (b, head, query i, key j) is kept iff word (j & 3) of
 *      Philox4x32-10(key = seed, counter = (i, j >> 2, head, b)) >= floor(p * 2^32): a pure function of the seed and the four indices,
 *      one 32-bit counter word each - no shape, tile or grid enters it, the forward, the backward and dg_xattn_keep_mask form the same
 *      mask, and no supported shape can wrap the counter (nothing is refused on its account).
 *  lse : fp32 (B, heads, Nq), the per-row log-sum-exp of the scaled scores (natural logarithm), the only thing the forward saves for
 *      the backward; NULL in the forward: not written
 *  workspace : dg_xattn_workspace_bytes(B, heads, Nq, Nk, backward) bytes (0 on bad arguments), 16-byte aligned: k and v (backward:
 *      and q and grad_out) as bf16 in MFMA fragment order, 7 KiB per (b, head, 32 rows), made by every call; backward: also
 *      rowsum(grad_out * out) and the log-sum-exp in log2 units, padded to whole tiles.  The backward needs nothing of the forward's.
 *  forward  : writes EVERY element of out (and of lse)
 *  backward : `out` and `lse` are the forward's results for the same q, k, v, scale, p and seed.  grad_q may be NULL (its kernel is
 *      not launched); grad_k and grad_v come from one kernel: both or neither.  Every element of a gradient that is given is written.
 *      Di = rowsum(dO * O); P re-formed from q, k and lse; dV = Pd^T dO; dS = P * (keep / (1 - p) * (dO V^T) - Di); dQ = scale dS K;
 *      dK = scale dS^T Q.
 *  dg_xattn_keep_mask : the keep decisions of (seed, p) as bytes (1 = kept), out uint8 (B, heads, Nq, Nk); all ones for p = 0
 * Arithmetic: q, k, v and grad_out rounded to bf16 (nearest even), products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; scores,
 * running maximum, exponentials, row sums, Di and the dropout scale in fp32; P and dS rounded to bf16 for the products that follow.
 * No atomics: every output element has one owner that sums in a fixed order, so two calls give the same bits.  No host
 * synchronisation.  Nothing outside the tensors and the workspace is read or written.
 */
size_t dg_xattn_workspace_bytes(int32_t B, int32_t heads, int32_t Nq, int32_t Nk, int32_t backward);
int dg_xattn_forward(const float* q, const float* k, const float* v, int32_t B, int32_t heads, int32_t Nq, int32_t Nk, int32_t head_dim,
                     float scale, float p, uint64_t seed, float* out, float* lse, void* workspace, size_t workspace_bytes,
                     dg_stream_t stream);
int dg_xattn_backward(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* grad_out,
                      int32_t B, int32_t heads, int32_t Nq, int32_t Nk, int32_t head_dim, float scale, float p, uint64_t seed,
                      float* grad_q, float* grad_k, float* grad_v, void* workspace, size_t workspace_bytes, dg_stream_t stream);
int dg_xattn_keep_mask(uint64_t seed, int32_t B, int32_t heads, int32_t Nq, int32_t Nk, float p, uint8_t* out, dg_stream_t stream);

/*
 * GPU batch augmentation: the dataset's augmented view `img_aug` and its coordinate map `coord_aug` (src/data.py:1082-1139;
 * src/train_segmentation.py:602-610) of a whole batch, every image under its own parameters, in two launches (dg_augment.hip):
 *      flip -> crop `box` -> bilinear resize to (h, w) (align_corners=False, taps held inside the crop; a box never exceeds the image,
 *      so this is never a down-scale) -> the record's colour ops in slot order -> RandomGrayscale -> 5 x 5 Gaussian blur (reflect pad)
 * with the arithmetic of torchvision's tensor transforms, and the same flip, crop and resize on meshgrid(linspace(-1,1,H),
 * linspace(-1,1,W)): coord_aug channel 0 is the row coordinate (aug_loss.crop_flip_coords's rule, bit for bit).
 *  img : fp32 (B, 3, H, W); its four element strides are passed and must be those of a contiguous tensor (DG_ERR_UNSUPPORTED otherwise)
 *  records_host : HOST memory, B records of 16 32-bit words: 0 flip (0 / 1), 1-4 the crop (top, left, height, width) in whole pixels of
 *      the flipped image, 5-8 the op of each slot (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none), 9-12 the four factors as
 *      fp32 indexed by op id, 13 gray (0 / 1), 14 blur sigma as fp32 (0: no blur), 15 zero.  Read by this call, on the host, for its
 *      checks and to decide whether the statistics kernel is launched; not kept.
 *  params : DEVICE memory, 4-byte aligned: a copy of the same B records followed by the H floats of linspace(-1, 1, H) and the W
 *      floats of linspace(-1, 1, W) - what the kernels read.  (The kernels hold every index inside the image whatever it says.)
 *  mean, stdv : HOST memory, three floats each, or both NULL.  NULL: the ops act on the tensor as given (the reference feeds them the
 *      ImageNet-normalised image; their clamps to [0, 1] act on those values).  Given: x * stdv + mean behind the resize and
 *      (x - mean) / stdv at the very end, per channel.
 *  img_aug : fp32 (B, 3, h, w);  coord_aug : fp32 (B, h, w, 2) - EVERY element of both is written
 *  workspace : dg_augment_workspace_bytes(B, h, w) bytes (0: sizes outside the limits below), 16-byte aligned: the fp64 partial sums
 *      of the contrast op's image mean, at most 64 per image, added in block order.  Nothing is kept between calls.
 * Ops: brightness clamp(f x, 0, 1); contrast clamp(f x + (1 - f) m, 0, 1) with m the mean over the image of gray(x) as the image
 * stands when the op's turn comes (one contrast op per image at most); saturation clamp(f x + (1 - f) gray(x), 0, 1); gray(x) =
 * 0.2989 r + 0.587 g + 0.114 b; hue: torchvision's _rgb2hsv, h = (h + f) mod 1, _hsv2rgb (p, q, t clamped to [0, 1]).
 * Refused before any launch: DG_ERR_UNSUPPORTED for C != 3, a side of the image or of the output below 3 (reflect padding by 2 needs
 * three pixels) or above 16384, B > 65535, a box outside the image, two contrast ops in one record, a non-contiguous img;
 * DG_ERR_INVALID for null or misaligned pointers, an op id outside -1 .. 3, a negative or non-finite sigma, std <= 0;
 * DG_ERR_WORKSPACE for a workspace that is too small.  Arithmetic: source positions fp64, everything behind them fp32 with one
 * rounding per operation (the blur's weights, products and sum are fp64, rounded once per pixel), the image mean fp64.  No atomics:
 * two calls give the same bits.  No host synchronisation, no allocation.
 */
size_t dg_augment_workspace_bytes(int32_t B, int32_t h, int32_t w);
int dg_augment_forward(const float* img, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w,
                       const int32_t* records_host, const void* params, const float* mean, const float* stdv, int32_t B, int32_t C,
                       int32_t H, int32_t W, int32_t h, int32_t w, float* img_aug, float* coord_aug, void* workspace,
                       size_t workspace_bytes, dg_stream_t stream);

/*
 * Batch preparation: the loader transform of the training data path (src/utils.py:164-182: Resize(res, NEAREST), the cropper, then
 * ToTensor and Normalize on the image, ToTargetTensor on the label and the depth map) for a whole batch - the samples and their kNN
 * positives, N = 2B - in ONE launch (dg_batch.hip), from the decoded uint8 planes of every sample at their own sizes.
 *  packed : uint8 device buffer of packed_bytes bytes: images RGB HWC, labels and depth maps HW, at the byte offsets the records name
 *  records_host : HOST memory, n_records records of 8 32-bit words, one per output plane group:
 *      0 kind (below), 1 sample n in [0, N), 2-3 byte offset of the source plane in `packed` (low, high word), 4 source width,
 *      5 source height, 6 label offset (added to the label byte; the value of DG_BATCH_LABEL_FILL), 7 mask rule (label kinds)
 *  tables_host : HOST memory, per sample W + H int32: xs[W], the source column of every output column, then ys[H], the source row of
 *      every output row - the resize and the crop composed by the caller (depthg_amd/data.py loader_index_tables).  Every record of
 *      sample n reads sample n's tables, so its planes must have one size.
 *  params : the DEVICE copy of both: the records, then the tables (one upload).  The host copies are read by this call for its checks.
 *  mean, stdv : HOST memory, three floats each
 *  img : fp32 (N,3,H,W) = (byte / 255 - mean[c]) / stdv[c], each operation rounded to float32 with IEEE division and no contraction,
 *      in ToTensor's and Normalize's order: the bits of torch's CPU chain
 *  label : int64 (N,H,W) = byte + label offset.  mask (N,H,W): by the records' rule (all label records of a call share one) bool bytes
 *      label == -1 (DG_BATCH_MASK_BOOL_IGNORED, src/data.py:900-902) or fp32 label > 0 (DG_BATCH_MASK_FLOAT_POSITIVE, src/data.py:128)
 *  depth : fp32 (N,H,W) = the byte value (DG_BATCH_DEPTH) or 255 (DG_BATCH_DEPTH_PLANE, src/data.py:897-898: no source is read)
 * An output no record writes may be NULL.  For every other output the records must name each sample exactly once, so EVERY element
 * is written, by one lane: no atomics, no intermediate image, two calls give the same bytes.  A lane owns four neighbouring columns
 * of a row and stores whole 16-byte vectors (the bool mask: one 4-byte word).  No workspace, no allocation, no host synchronisation.
 * Refused before any launch, with the reason in dg_last_error: DG_ERR_INVALID for null pointers, an unknown kind or mask rule, mixed
 * mask rules, a sample outside [0, N), a zero-sized source plane, a plane that leaves `packed`, a table entry outside its plane
 * (the plane is narrower than the tables address), an output that is not 16-byte aligned, a sample written twice or not at all,
 * std <= 0; DG_ERR_UNSUPPORTED for W not a multiple of 4, a side of a source plane or of the output above 16384, N or n_records
 * above 65535.
 */
#define DG_BATCH_IMAGE       0   /* RGB uint8 HWC -> img */
#define DG_BATCH_LABEL       1   /* uint8 HW -> label and mask */
#define DG_BATCH_DEPTH       2   /* uint8 HW -> depth */
#define DG_BATCH_DEPTH_PLANE 3   /* no source: depth = 255 */
#define DG_BATCH_LABEL_FILL  4   /* no source: label = label offset, and its mask (src/data.py:126: a folder without labels) */
#define DG_BATCH_MASK_BOOL_IGNORED   0
#define DG_BATCH_MASK_FLOAT_POSITIVE 1
int dg_batch_prep(const uint8_t* packed, size_t packed_bytes, const int32_t* records_host, const int32_t* tables_host,
                  const void* params, int32_t n_records, int32_t N, int32_t H, int32_t W, const float* mean, const float* stdv,
                  float* img, int64_t* label, void* mask, float* depth, dg_stream_t stream);

/*
 * Frozen-backbone feature cache (dg_feat_cache.hip).  The backbone is frozen, runs in eval mode and draws nothing (src/modules.py:90-137:
 * `image_feat` under no_grad), and a deterministic loader transform feeds it, so the `image_feat` of train image i that the step's two
 * featurizer passes recompute every epoch (src/train_segmentation.py:194-212) is one tensor: it is stored once and read back per batch.
 *  cache : (N, L) rows, L = C h w, of `dtype` (below) on the device; row i = image_feat of image i, flattened
 * dg_featcache_put (k_fc_put): rows idx[0..n) of the cache = src (n, L) fp32 converted to `dtype` - DG_FC_F32 a copy, DG_FC_F16 and
 *  DG_FC_BF16 round to nearest even with the bits of torch's .to(dtype) on a tensor: infinities stay, overflow rounds to infinity,
 *  fp16 subnormals are formed, a fp16 NaN keeps its sign and the top ten payload bits and is quiet, EVERY bf16 NaN is 0xFFFF
 *  (what torch's vectorised CPU cast stores; c10::BFloat16's scalar constructor gives 0x7FC0 - both are quiet NaNs).
 *  The caller gives each row once per call (two lanes would race for it otherwise); the entry cannot see that: the index lives on the device.
 * dg_featcache_gather (k_fc_gather): out (2n, L) fp32, rows 0..n-1 = cache rows idx_a[0..n), rows n..2n-1 = cache rows idx_b[0..n),
 *  widened exactly - ONE launch and one allocation for a batch and its positives, laid out as the head's paired pass takes its two
 *  maps (dg_head_forward's feats / feats_pos = out and out + n L).  idx_b may be NULL: out is (n, L).  An index may repeat, within a
 *  list and between the two.
 * idx, idx_a, idx_b : int64 on the DEVICE, read by the kernels.  The caller checks them on the host beforehand; a row index outside
 *  [0, N) is never dereferenced all the same: that row is skipped (in gather its output row stays unwritten).
 * Both kernels stream: a lane moves 16 bytes of the cache per access (eight 16-bit elements = two 16-byte fp32 accesses, or four fp32)
 * wherever the cache row and the fp32 row reach a 16-byte boundary at the same element, one element per lane in front of that boundary
 * and behind the last whole vector - and over the whole row where they never do (L need not be a multiple of 8).  No LDS, no atomics,
 * no workspace, no allocation, no host synchronisation; every element of the rows named is written exactly once, two calls give the
 * same bytes.  Refused before any launch: DG_ERR_INVALID for an unknown dtype, N < 1, L < 1, n < 0, null or misaligned pointers (the
 * cache on its element size, fp32 tensors on 4 bytes, indices on 8); DG_ERR_UNSUPPORTED for more than 65535 rows a call.  n == 0: nothing.
 */
#define DG_FC_F32  0
#define DG_FC_F16  1
#define DG_FC_BF16 2
int dg_featcache_put(void* cache, int32_t dtype, int64_t N, int64_t L, const float* src, const int64_t* idx, int64_t n,
                     dg_stream_t stream);
int dg_featcache_gather(const void* cache, int32_t dtype, int64_t N, int64_t L, const int64_t* idx_a, const int64_t* idx_b, int64_t n,
                        float* out, dg_stream_t stream);

/*
 * Device-resident sample cache (dg_sample_cache.hip).  With a deterministic loader crop the resized and cropped bytes of every image,
 * label and depth map (src/utils.py:164-182) are the same in every epoch, and the reference's datasets form their tensors from those
 * bytes alone (src/data.py:894-902, :126-128): they are stored once on the card and a batch comes back from them without a file, a
 * decoder, a pinned buffer or an upload.
 *  cache : uint8 (n_images, planes, H, W) on the device at the loader's OUTPUT size, W a multiple of 4, 4-byte aligned.  planes =
 *      3 + has_labels + with_depth in the order R, G, B, label (has_labels), depth (with_depth).
 * dg_samplecache_put, kernel k_sc_put: packed / packed_bytes / records_host / tables_host / params / n_records exactly as dg_batch_prep
 *  takes them for n samples, and idx: int64 on the DEVICE, the cache row of each sample, each row once per call.  Writes the BYTES the
 *  nearest resize and crop select - k_batch_prep's geometry without its arithmetic: image HWC becomes three planes, a
 *  DG_BATCH_DEPTH_PLANE record stores the byte 255, a DG_BATCH_LABEL_FILL record writes nothing.  Every sample needs one image record,
 *  one DG_BATCH_LABEL record iff has_labels and one depth record iff with_depth, so every byte of every named row is written once.
 * dg_samplecache_gather, kernel k_sc_gather: ONE launch writes rows 0..n-1 from idx_a and rows n..2n-1 from idx_b (int64 on the DEVICE;
 *  idx_b may be NULL: n rows; an index may repeat, within a list and between the two) of every output that is not NULL:
 *      img   fp32 (rows,3,H,W) = (byte / 255 - mean[c]) / stdv[c] through the device function dg_batch_prep's kernel uses: its bits
 *      label int64 (rows,H,W)  = byte + label_offset, or `fill` for a cache without a label plane
 *      mask  (rows,H,W)        = fp32 label > 0 (DG_BATCH_MASK_FLOAT_POSITIVE) or bool bytes label == -1 (DG_BATCH_MASK_BOOL_IGNORED)
 *      depth fp32 (rows,H,W)   = the byte value
 *  mean, stdv : HOST memory, three floats each (needed with img).  A lane owns four neighbouring pixels of a row: one 32-bit load per
 *  plane, 16-byte stores (the bool mask: one 4-byte word).
 * No LDS in the gather, no atomics, no workspace, no allocation, no host synchronisation; two calls give the same bytes.  The callers
 * check the indices on the host; a row index outside [0, n_images) is never dereferenced all the same: that row is skipped.
 * Refused before any launch: DG_ERR_INVALID for null or misaligned pointers (the cache on 4 bytes, indices on 8, outputs on 16), sizes
 * that are not positive, an unknown record kind or mask rule, a record that does not fit the cache's planes, a plane group written
 * twice or not at all, a source plane that leaves `packed` or is smaller than its tables address, depth asked of a cache without a
 * depth plane, no output asked for, std <= 0; DG_ERR_UNSUPPORTED for W not a multiple of 4, a side above 16384, more than 65535 rows or
 * records a call.  n == 0: nothing.
 */
int dg_samplecache_put(uint8_t* cache, int64_t n_images, int32_t has_labels, int32_t with_depth, int32_t H, int32_t W, const int64_t* idx,
                       int32_t n, const uint8_t* packed, size_t packed_bytes, const int32_t* records_host, const int32_t* tables_host,
                       const void* params, int32_t n_records, dg_stream_t stream);
int dg_samplecache_gather(const uint8_t* cache, int64_t n_images, int32_t has_labels, int32_t with_depth, int32_t H, int32_t W,
                          const int64_t* idx_a, const int64_t* idx_b, int32_t n, const float* mean, const float* stdv, int32_t label_offset,
                          int32_t fill, int32_t mask_rule, float* img, int64_t* label, void* mask, float* depth, dg_stream_t stream);

/*
 * The batch draw of a cached training step on the device (dg_epoch.hip, kernel k_epoch_draw).  It replaces, for a batch of B,
 * src/data.py:1073-1080:
 *      def __getitem__(self, ind):
 *          pack = self.dataset[ind]
 *          if self.pos_images or self.pos_labels:
 *              ind_pos = self.nns[ind][torch.randint(low=1, high=self.num_neighbors + 1, size=[]).item()]
 *              pack_pos = self.dataset[ind_pos]
 * - B host draws with a synchronisation each, and the sampler's index list behind them - by ONE launch whose operands all live on the
 * device, so that a step recorded in a hipGraph draws its next batch at every replay:
 *  state   : {seed, draws, cursor}, three 64-bit words on the DEVICE, owned by the caller.  The words are laid out as the generator
 *            state of dg_super_perms is, but the third is this entry's cursor, not a ticket: give this entry a state of its own.
 *  order   : int64 (n_images,) on the device, the epoch's visiting order (a permutation of 0..n_images-1)
 *  nns     : int64 (n_images, K) on the device, the nearest-neighbour table; column 0 is the image itself
 *  ind, ind_pos : int64 (B,) on the device, every element written, with plain vector stores
 * Slot j: ind[j] = order[cursor + j]; r = 1 + u % num_neighbors with u = word 0 of Philox4x32-10 (dg_device.h) keyed by `seed` at the
 * 128-bit counter (draws + j, 0); ind_pos[j] = nns[ind[j]][r].  After every slot has read the state one thread stores cursor + B and
 * draws + B.  The positives are a uniform draw from columns 1..num_neighbors as the reference's are, but NOT torch.randint's stream.
 * One block: B <= 1024.  No LDS, no atomics, no workspace, no allocation, no host synchronisation.
 * Refused before any launch: DG_ERR_INVALID for B, n_images or K < 1, num_neighbors < 1 or >= K, null or misaligned (8 bytes)
 * pointers; DG_ERR_UNSUPPORTED for B > 1024.  cursor + B <= n_images is the CALLER's invariant (the cursor cannot be read here
 * without a synchronisation): the kernel holds its position in `order` at n_images - 1 and the table row inside [0, n_images), so a
 * broken invariant repeats an entry and never reads outside the two buffers.
 */
int dg_epoch_draw(uint64_t* state, const int64_t* order, const int64_t* nns, int32_t B, int32_t num_neighbors, int64_t n_images, int32_t K,
                  int64_t* ind, int64_t* ind_pos, dg_stream_t stream);

/* Measurement aid: name of the kernel the fused correlation launch of this descriptor runs ("k_corr2": the one-wave-per-SIMD
 * form of dg_corr2.hip, "k_corr_main": the general form), decided by the same predicate the launch uses; NULL on a bad desc. */
const char* dg_corr_main_kernel_name(const dg_corr_desc* desc);

/* Measurement aid: 1 when the fused correlation launch of this descriptor also forms the intra pair-set's streamed-side code
 * gradient (k_corr2's FOLD: helper(feats, feats, code, code) of src/modules.py:1236-1254 is symmetric up to its row-mean centering;
 * DESIGN.md section 4.1) - that share of the algorithmic work then belongs to the fused launch, not to k_gs; 0 otherwise; -1 on a
 * bad desc.  (DG_FOLD_INTRA=0 in the environment switches the fold off: a test seam, see the switch list in dg_common.h.) */
int dg_corr_intra_folded(const dg_corr_desc* desc);

/*
 * Measurement aid (bench.py roofline leg): the execution span of the fused correlation launch INSIDE the step, hipGraph replays
 * included, and the shader clock its CUs held.  `span` = device pointer to FOUR uint64 (or NULL: off).  Every workgroup of the fused
 * kernel of every later dg_corr_forward* call of this process takes min(span[0], entry time) and max(span[1], exit time) and adds its
 * own lifetime to span[2] (shader cycles, s_memtime) and span[3] (ticks of the GPU's constant 100-MHz wall clock, s_memrealtime:
 * 10 ns per tick), all with device-scope atomics.  The caller sets {UINT64_MAX, 0, 0, 0} in front of the step it wants to read (e.g.
 * a copy on the launch stream) and reads behind it: (span[1] - span[0]) x 10 ns = the interval a kernel trace reports for the
 * launch, minus the dispatch ramp; span[2] / span[3] x 0.1 = the clock in GHz the kernel's CUs held on average.  Nothing in the
 * product path depends on it.  LIFETIME: the pointer in force when a launch is RECORDED is what the launch uses - a hipGraph captured
 * while a span was set writes to it at every replay, so the four words must outlive every such graph (or the graph must be dropped
 * first); capture the graphs you time with the span off (NULL) and a separate one with it on for the measurement.
 */
int dg_prof_main_span(void* span);

/*
 * Measurement aid (bench.py roofline leg): re-launch only the fused correlation kernel on the operands a
 * previous dg_corr_forward with the same desc / perms / workspace prepared.  Idempotent.
 */
int dg_corr_relaunch_main(const dg_corr_desc* desc, const int64_t* perms,
                          void* workspace, size_t workspace_bytes, dg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEPTHG_CORR_H */
