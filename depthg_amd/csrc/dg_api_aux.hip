// C ABI of the gfx950 DepthG library (include/depthg_corr.h), the units' shared state and the small subsystems: version and error
// text, the library's side stream, batch maps / random draws / coordinate samplers, kNN, LHP, fused Adam, ViT attention and linear, the fused depth encoder, the depth guidance's cross-attention.  (The auxiliary loss terms: dg_api_loss.hip; the training data path: dg_api_data.hip.)
// Host-side only: argument checks and kernel launches on the caller's stream.
#include "dg_api.h"
#include "dg_aux_args.h"
#include "dg_depth_args.h"
#include "dg_corr_args.h"     // the samplers of dg_post.hip: super_perms, rand_coords_state, fps

#include <cstdarg>
#include <map>

// ---- error reporting (dg_api.h)
thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" int dg_version(void) { return DG_VERSION; }
extern "C" const char* dg_last_error(void) { return g_err; }

// ---- the library's second stream (dg_api.h)
SideStream* side_stream_for(hipStream_t caller) {
    static std::mutex mu;
    static std::map<int, SideStream> table;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto it = table.find(dev);
    if (it != table.end()) return &it->second;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(caller, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};       // fork, join, two hand-overs from the side stream in mid-region
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    bool ok = true;
    for (int i = 0; i < 4 && ok; ++i) ok = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        for (int i = 0; i < 4; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);      // nothing half-made stays behind: the call launches in sequence instead
        (void)hipStreamDestroy(s);
        return nullptr;
    }
    SideStream& ss = table[dev];        // (std::map nodes do not move: the pointer stays valid; std::mutex is not copyable)
    ss.s = s; ss.fork = ev[0]; ss.join = ev[1]; ss.mid[0] = ev[2]; ss.mid[1] = ev[3];
    return &ss;
}

// the keys' source: `keys` (explicit), else `state` (the device-resident generator), else `seed`
extern "C" int dg_super_perms(const float* keys, uint64_t seed, uint64_t* state, int32_t count, int32_t B, int64_t* out, dg_stream_t stream_) {
    if (count < 0 || B < 1 || B > 8192) return fail(DG_ERR_INVALID, "dg_super_perms: count=%d B=%d outside the supported range", count, B);
    if (count == 0) return DG_OK;
    if (keys && state) return fail(DG_ERR_INVALID, "dg_super_perms: `keys` and `state` are two sources of the same keys: give one");
    if (!out) return fail(DG_ERR_INVALID, "null pointer");
    DG_HIP(dg_launch_super_perms(keys, seed, reinterpret_cast<unsigned long long*>(state), count, B, out, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_rand_coords_state(uint64_t* state, int64_t n, float* out, dg_stream_t stream_) {
    if (!state || !out) return fail(DG_ERR_INVALID, "null pointer");
    if (n < 1 || n > (1ll << 24)) return fail(DG_ERR_INVALID, "dg_rand_coords_state: n=%lld outside [1, 2^24]", (long long)n);
    DG_HIP(dg_launch_rand_coords_state(reinterpret_cast<unsigned long long*>(state), out, (int)n, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_rand_keep_state(uint64_t* state, int64_t n, float p_keep, float* out, dg_stream_t stream_) {
    if (!state || !out) return fail(DG_ERR_INVALID, "null pointer");
    if (n < 1 || n > (1ll << 24) || !(p_keep >= 0.f && p_keep <= 1.f)) return fail(DG_ERR_INVALID, "dg_rand_keep_state: n=%lld, p_keep=%g", (long long)n, (double)p_keep);
    DG_HIP(dg_launch_rand_coords_state(reinterpret_cast<unsigned long long*>(state), out, (int)n, static_cast<hipStream_t>(stream_), p_keep));
    return DG_OK;
}

extern "C" int dg_salience_coords(const float* salience, int32_t B, int32_t H, int32_t W, int32_t n, const float* u_sel,
                                  const float* u_fallback, float* out_coords, dg_stream_t stream_) {
    if (!salience || !u_sel || !u_fallback || !out_coords) return fail(DG_ERR_INVALID, "null pointer");
    if (B < 1 || H < 1 || W < 1 || n < 1) return fail(DG_ERR_INVALID, "bad salience sampler dimensions");
    if ((size_t)H * W > (1u << 24)) return fail(DG_ERR_UNSUPPORTED, "salience map %dx%d too large", H, W);
    DG_HIP(dg_launch_salience_coords(salience, B, H, W, n, u_sel, u_fallback, out_coords, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_simple_depth_coords(const float* depth, int32_t B, int32_t depth_h, int32_t depth_w, int32_t h, int32_t w,
                                      int32_t n, const float* u_value, const float* u_pick, float* out_coords,
                                      dg_stream_t stream_) {
    if (!depth || !u_value || !u_pick || !out_coords) return fail(DG_ERR_INVALID, "null pointer");
    if (B < 1 || h < 1 || w < 1 || n < 1 || depth_h < 1 || depth_w < 1) return fail(DG_ERR_INVALID, "bad sampler dimensions");
    if ((size_t)h * w > 4096) return fail(DG_ERR_UNSUPPORTED, "feature map %dx%d too large for the sampler (max 4096 pixels)", h, w);
    DG_HIP(dg_launch_simple_coords(depth, B, depth_h, depth_w, h, w, n, u_value, u_pick, out_coords,
                                   static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_knn_similarities(const float* queries, const float* feats, int64_t rows_q, int64_t n, int32_t F, int64_t q_stride,
                                   int64_t f_stride, float* out, int64_t out_stride, dg_stream_t stream_) {
    if (rows_q < 0 || n < 0 || F < 1 || q_stride < F || f_stride < F || out_stride < n) return fail(DG_ERR_INVALID, "bad similarity dimensions");
    if (rows_q == 0 || n == 0) return DG_OK;
    if (!queries || !feats || !out) return fail(DG_ERR_INVALID, "null pointer");
    if (n > 65535ll * 128) return fail(DG_ERR_UNSUPPORTED, "more than 8,388,480 candidate rows per call");
    DG_HIP(dg_launch_sims_nt(queries, feats, rows_q, n, F, q_stride, f_stride, out, out_stride, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_topk_rows(const float* vals, int64_t rows, int64_t cols, int64_t row_stride, int32_t k, int64_t* out_idx,
                            float* out_val, dg_stream_t stream_) {
    if (rows < 0 || cols < 1 || k < 1 || row_stride < cols) return fail(DG_ERR_INVALID, "bad top-k dimensions");
    if (k > 64 || k > cols) return fail(DG_ERR_UNSUPPORTED, "top-k needs k <= 64 and k <= cols (k=%d, cols=%lld)", k, (long long)cols);
    if (cols >= (1ll << 32) || rows >= (1ll << 31)) return fail(DG_ERR_UNSUPPORTED, "similarity matrix too large");
    if (rows == 0) return DG_OK;
    if (!vals || !out_idx) return fail(DG_ERR_INVALID, "null pointer");
    DG_HIP(dg_launch_topk_rows(vals, rows, cols, row_stride, k, reinterpret_cast<long long*>(out_idx), out_val,
                               static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

static int lhp_check(int32_t B, int32_t D, int32_t h, int32_t w) {
    if (B < 1 || D < 1 || h < 1 || w < 1) return fail(DG_ERR_INVALID, "bad LHP dimensions");
    if (D > 128) return fail(DG_ERR_UNSUPPORTED, "D=%d > 128 code channels not supported", D);
    if ((size_t)h * w > 4096) return fail(DG_ERR_UNSUPPORTED, "feature map %dx%d too large for the LHP propagation (max 4096 positions)", h, w);
    return DG_OK;
}

extern "C" int dg_lhp_forward(const float* code, const float* depth, int32_t B, int32_t D, int32_t h, int32_t w, int32_t depth_h,
                              int32_t depth_w, float* out, float* points, float* stats, dg_stream_t stream_) {
    if (int rc = lhp_check(B, D, h, w)) return rc;
    if (depth_h < 1 || depth_w < 1) return fail(DG_ERR_INVALID, "bad depth size");
    if (!code || !depth || !out || !points || !stats) return fail(DG_ERR_INVALID, "null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const uint32_t bits = 0x404f54cbu;            // 2*tan(90/2 rad), the reference's float32 factor (dg_fps_coords)
    float factor;
    memcpy(&factor, &bits, 4);
    DG_HIP(dg_launch_lhp_points(depth, B, depth_h, depth_w, h, w, factor, points, s));
    DG_HIP(dg_launch_lhp_propagate(false, code, points, stats, B, D, h * w, out, s));
    return DG_OK;
}

extern "C" int dg_lhp_backward(const float* grad_out, const float* points, const float* stats, int32_t B, int32_t D, int32_t h,
                               int32_t w, float* grad_code, dg_stream_t stream_) {
    if (int rc = lhp_check(B, D, h, w)) return rc;
    if (!grad_out || !points || !stats || !grad_code) return fail(DG_ERR_INVALID, "null pointer");
    DG_HIP(dg_launch_lhp_propagate(true, grad_out, points, const_cast<float*>(stats), B, D, h * w, grad_code,
                                   static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_lhp_map_forward(int32_t mode, const float* code, const float* attn, const float* depth, const float* divide,
                                  int32_t B, int32_t D, int32_t h, int32_t w, int32_t heads, int32_t depth_h, int32_t depth_w,
                                  float* out, float* map, float* points, dg_stream_t stream_) {
    if (int rc = lhp_check(B, D, h, w)) return rc;
    if (mode < DG_LHP_ATTN || mode > DG_LHP_ORIG_ATTN) return fail(DG_ERR_INVALID, "unknown LHP map mode %d", mode);
    if (!code || !out) return fail(DG_ERR_INVALID, "null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (mode == DG_LHP_ORIG_DEPTH) {
        if (!depth || !points || depth_h < 1 || depth_w < 1) return fail(DG_ERR_INVALID, "the depth map and the points scratch are required");
        const uint32_t bits = 0x404f54cbu;        // 2*tan(90/2 rad), as in dg_lhp_forward
        float factor;
        memcpy(&factor, &bits, 4);
        DG_HIP(dg_launch_lhp_points(depth, B, depth_h, depth_w, h, w, factor, points, s));
    } else if (!attn || heads < 1) {
        return fail(DG_ERR_INVALID, "the attention tensor (B,heads,h*w+1,h*w+1) is required");
    }
    if (!map) return fail(DG_ERR_INVALID, "the map buffer is required");
    if (mode != DG_LHP_ATTN && !divide) return fail(DG_ERR_INVALID, "divide_num is required");
    DG_HIP(dg_launch_lhp_map(mode, code, attn, points, divide, B, D, h, w, heads, out, map, s));
    return DG_OK;
}

extern "C" int dg_lhp_map_backward(int32_t mode, const float* grad_out, const float* map, const float* divide, int32_t B, int32_t D,
                                   int32_t h, int32_t w, float* grad_code, dg_stream_t stream_) {
    if (int rc = lhp_check(B, D, h, w)) return rc;
    if (mode < DG_LHP_ATTN || mode > DG_LHP_ORIG_ATTN) return fail(DG_ERR_INVALID, "unknown LHP map mode %d", mode);
    if (!grad_out || !map || !grad_code || (mode != DG_LHP_ATTN && !divide)) return fail(DG_ERR_INVALID, "null pointer");
    DG_HIP(dg_launch_lhp_map_bwd(mode, grad_out, map, divide, B, D, h, w, grad_code, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" size_t dg_fps_workspace_bytes(int32_t B, int32_t h, int32_t w) {
    // the pooled depth maps of B images (adaptive_avg_pool2d to the feature map, written by a launch over the whole chip in front of
    // the sampler); the sampler itself keeps its state in LDS
    if (B < 1 || h < 1 || w < 1) return 256;
    return (size_t)B * h * w * 4 + 256;
}

// depth_pos non-null: the B maps of a second tensor behind the first's (the anchors' depth, then the positives'), nB = 2 B maps in all
extern "C" int dg_fps_coords(const float* depth, const float* depth_pos, int32_t B, int32_t depth_h, int32_t depth_w, int32_t h, int32_t w,
                             int32_t S, float* out_coords, int32_t* out_inds, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!depth || !out_coords) return fail(DG_ERR_INVALID, "null pointer");
    const int32_t nB = depth_pos ? 2 * B : B;
    if (nB < 1 || B < 1 || h < 1 || w < 1 || S < 1 || depth_h < h || depth_w < w) return fail(DG_ERR_INVALID, "bad FPS dimensions");
    if (S * S > h * w) return fail(DG_ERR_INVALID, "cannot sample %d points from a %dx%d map", S * S, h, w);
    if ((size_t)h * w > 4096) return fail(DG_ERR_UNSUPPORTED, "feature map %dx%d too large for the sampler (max 4096 pixels)", h, w);
    // 2*tan(fov/2) with fov = 90 taken in radians (reference quirk, src/modules.py:989,1016), float32 bits
    const uint32_t bits = 0x404f54cbu;
    float factor;
    memcpy(&factor, &bits, 4);
    // (a workspace that is missing or too small is not an error: the sampler then pools inside its own blocks, one image per CU)
    float* pooled = (workspace && workspace_bytes >= (size_t)nB * h * w * 4) ? static_cast<float*>(workspace) : nullptr;
    DG_HIP(dg_launch_fps(depth, depth_pos, B, nB, depth_h, depth_w, h, w, S, factor, out_coords, out_inds, pooled, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" size_t dg_fps_feats_workspace_bytes(int32_t B, int32_t h, int32_t w) { return dg_fps_workspace_bytes(B, h, w); }      // the pooled depth maps

// dg_fps_coords with the feature term of fps_depth_feats (src/modules.py:1124-1180); depth_pos and feats_pos come together or not at all
extern "C" int dg_fps_feats_coords(const float* depth, const float* depth_pos, const float* feats, const float* feats_pos, int32_t B, int32_t C,
                                   int32_t depth_h, int32_t depth_w, int32_t h, int32_t w, int32_t S, float* out_coords, int32_t* out_inds,
                                   void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!depth || !feats || !out_coords || !workspace) return fail(DG_ERR_INVALID, "dg_fps_feats_coords: null pointer");
    if ((depth_pos == nullptr) != (feats_pos == nullptr)) return fail(DG_ERR_INVALID, "dg_fps_feats_coords: depth_pos and feats_pos come together");
    if (((uintptr_t)depth | (uintptr_t)depth_pos | (uintptr_t)feats | (uintptr_t)feats_pos | (uintptr_t)out_coords | (uintptr_t)out_inds |
         (uintptr_t)workspace) & 3)
        return fail(DG_ERR_INVALID, "dg_fps_feats_coords: pointers must be 4-byte aligned");
    if (B < 1 || B > (1 << 20) || h < 1 || w < 1 || S < 1 || depth_h < h || depth_w < w) return fail(DG_ERR_INVALID, "bad FPS dimensions");
    if (C < 1) return fail(DG_ERR_INVALID, "dg_fps_feats_coords: C=%d feature channels", C);
    const int32_t nB = depth_pos ? 2 * B : B;
    if ((size_t)h * w > 4096) return fail(DG_ERR_UNSUPPORTED, "feature map %dx%d too large for the sampler (max 4096 pixels)", h, w);
    if ((int64_t)S * S > (int64_t)h * w) return fail(DG_ERR_INVALID, "cannot sample %lld points from a %dx%d map", (long long)S * S, h, w);
    if (C > 16384) return fail(DG_ERR_UNSUPPORTED, "dg_fps_feats_coords: C=%d > 16384 feature channels (the last point's row lives in LDS)", C);
    if (!dg_pool_depth_fits(depth_h, depth_w, h))
        return fail(DG_ERR_UNSUPPORTED, "dg_fps_feats_coords: the %d-wide depth rows of one pooled row exceed 64 KB of LDS", depth_w);
    if (workspace_bytes < (size_t)nB * h * w * 4) return fail(DG_ERR_WORKSPACE, "dg_fps_feats_coords: workspace too small (dg_fps_feats_workspace_bytes)");
    const uint32_t bits = 0x404f54cbu;            // 2*tan(90/2 rad), the reference's float32 factor (dg_fps_coords)
    float factor;
    memcpy(&factor, &bits, 4);
    DG_HIP(dg_launch_fps_feats(depth, depth_pos, feats, feats_pos, B, nB, C, depth_h, depth_w, h, w, S, factor, out_coords, out_inds,
                               static_cast<float*>(workspace), static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// The pooled depth maps of the large sampler (written only where the depth maps are larger than the grid)
extern "C" size_t dg_fps_large_workspace_bytes(int32_t B, int32_t h, int32_t w) {
    if (B < 1 || h < 1 || w < 1 || (int64_t)h * w > DG_FPS_LARGE_MAX_POS) return 256;
    return (size_t)B * h * w * 4 + 256;
}

// dg_fps_coords on pooled grids of up to 65536 positions (k_fps_large): the same selection, bit for bit, on every grid both serve
extern "C" int dg_fps_coords_large(const float* depth, const float* depth_pos, int32_t B, int32_t depth_h, int32_t depth_w, int32_t h, int32_t w,
                                   int32_t S, float* out_coords, int32_t* out_inds, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!depth || !out_coords) return fail(DG_ERR_INVALID, "dg_fps_coords_large: null pointer");
    if (((uintptr_t)depth | (uintptr_t)depth_pos | (uintptr_t)out_coords | (uintptr_t)out_inds | (uintptr_t)workspace) & 3)
        return fail(DG_ERR_INVALID, "dg_fps_coords_large: pointers must be 4-byte aligned");
    if (B < 1 || B > (1 << 20) || h < 1 || w < 1 || S < 1 || depth_h < h || depth_w < w) return fail(DG_ERR_INVALID, "dg_fps_coords_large: bad FPS dimensions");
    const int32_t nB = depth_pos ? 2 * B : B;
    if ((int64_t)h * w > DG_FPS_LARGE_MAX_POS)
        return fail(DG_ERR_UNSUPPORTED, "dg_fps_coords_large: grid %dx%d too large for the sampler (max %d positions)", h, w, DG_FPS_LARGE_MAX_POS);
    if ((int64_t)S * S > (int64_t)h * w) return fail(DG_ERR_INVALID, "dg_fps_coords_large: cannot sample %lld points from a %dx%d map", (long long)S * S, h, w);
    if ((int64_t)S * S > DG_FPS_LARGE_MAX_SEL)
        return fail(DG_ERR_UNSUPPORTED, "dg_fps_coords_large: %lld selections exceed the %d the block's selection table holds", (long long)S * S, DG_FPS_LARGE_MAX_SEL);
    const bool pooling = depth_h != h || depth_w != w;
    if (pooling && !dg_pool_depth_fits(depth_h, depth_w, h))
        return fail(DG_ERR_UNSUPPORTED, "dg_fps_coords_large: the %d-wide depth rows of one pooled row exceed 64 KB of LDS", depth_w);
    if (pooling && (!workspace || workspace_bytes < (size_t)nB * h * w * 4))
        return fail(DG_ERR_WORKSPACE, "dg_fps_coords_large: workspace too small for the pooled depth maps (dg_fps_large_workspace_bytes)");
    const uint32_t bits = 0x404f54cbu;            // 2*tan(90/2 rad), the reference's float32 factor (dg_fps_coords)
    float factor;
    memcpy(&factor, &bits, 4);
    DG_HIP(dg_launch_fps_large(depth, depth_pos, B, nB, depth_h, depth_w, h, w, S, factor, out_coords, out_inds, static_cast<float*>(workspace),
                               static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// label_pos non-null: the B label maps of a second tensor behind the first's, 2 B images of ONE output in one launch
extern "C" int dg_label_onehot(const int64_t* label, const int64_t* label_pos, int32_t B, int32_t n_classes, int32_t H, int32_t W, float* out,
                               dg_stream_t stream_) {
    if (!label || !out) return fail(DG_ERR_INVALID, "dg_label_onehot: null pointer");
    if (((uintptr_t)label | (uintptr_t)label_pos) & 7) return fail(DG_ERR_INVALID, "dg_label_onehot: the label maps must be 8-byte aligned");
    if ((uintptr_t)out & 3) return fail(DG_ERR_INVALID, "dg_label_onehot: `out` must be 4-byte aligned");
    if (B < 1 || H < 1 || W < 1 || n_classes < 0) return fail(DG_ERR_INVALID, "dg_label_onehot: B=%d n_classes=%d map %dx%d", B, n_classes, H, W);
    if (n_classes + 1 > 256) return fail(DG_ERR_UNSUPPORTED, "dg_label_onehot: n_classes + 1 = %d > 256 channels", n_classes + 1);
    const int64_t nB = label_pos ? 2 * (int64_t)B : B;
    if (nB > 65535) return fail(DG_ERR_UNSUPPORTED, "dg_label_onehot: %lld images in one launch (max 65535)", (long long)nB);
    if ((int64_t)H * W > (1 << 24)) return fail(DG_ERR_UNSUPPORTED, "dg_label_onehot: map %dx%d too large (max 2^24 pixels)", H, W);
    DG_HIP(dg_launch_label_onehot(label, label_pos, B, (int)nB, n_classes + 1, H, W, out, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- the optimisation step's Adams (dg_optim.hip)
extern "C" int dg_adam_step(const dg_adam_seg* segs, int32_t n_seg, const dg_adam_group* groups, int32_t n_groups, int32_t device_steps,
                            void* tickets, dg_stream_t stream_) {
    if (!segs || !groups) return fail(DG_ERR_INVALID, "dg_adam_step: null table");
    if (n_seg < 1 || n_groups < 1) return fail(DG_ERR_INVALID, "dg_adam_step: n_seg=%d, n_groups=%d must be positive", n_seg, n_groups);
    if (n_groups > DG_ADAM_MAX_GROUPS) return fail(DG_ERR_UNSUPPORTED, "dg_adam_step: %d groups (max %d per call)", n_groups, DG_ADAM_MAX_GROUPS);
    for (int k = 0; k < n_groups; ++k) {
        const dg_adam_group& g = groups[k];
        if (!(g.lr >= 0.0) || !(g.beta1 >= 0.0 && g.beta1 < 1.0) || !(g.beta2 >= 0.0 && g.beta2 < 1.0) || !(g.eps >= 0.0))
            return fail(DG_ERR_INVALID, "dg_adam_step: group %d: lr=%g betas=(%g, %g) eps=%g", k, g.lr, g.beta1, g.beta2, g.eps);
    }
    for (int k = 0; k < n_seg; ++k) {
        const dg_adam_seg& s = segs[k];
        if (!s.param || !s.exp_avg || !s.exp_avg_sq) return fail(DG_ERR_INVALID, "dg_adam_step: segment %d: null parameter / state pointer", k);
        if (s.numel < 1 || s.numel > 0x7fffffffll) return fail(DG_ERR_INVALID, "dg_adam_step: segment %d: numel=%lld outside [1, 2^31)", k, (long long)s.numel);
        if (s.group < 0 || s.group >= n_groups) return fail(DG_ERR_INVALID, "dg_adam_step: segment %d: group %d of %d", k, s.group, n_groups);
        if (((uintptr_t)s.param | (uintptr_t)s.grad | (uintptr_t)s.exp_avg | (uintptr_t)s.exp_avg_sq) & 3)
            return fail(DG_ERR_INVALID, "dg_adam_step: segment %d: a pointer is not 4-byte aligned", k);
        if (device_steps) {
            if (!s.step_dev || ((uintptr_t)s.step_dev & 3)) return fail(DG_ERR_INVALID, "dg_adam_step: segment %d: step_dev must be a device float", k);
            if (s.numel > DG_ADAM_CHUNK && !tickets) return fail(DG_ERR_INVALID, "dg_adam_step: segment %d spans several blocks: tickets must be given", k);
        } else if (!(s.step_host >= 1.0)) {
            return fail(DG_ERR_INVALID, "dg_adam_step: segment %d: step_host=%g (the count after this step) must be >= 1", k, s.step_host);
        }
    }
    for (int k0 = 0; k0 < n_seg; k0 += DG_ADAM_MAX_SEGS) {
        const int c = n_seg - k0 < DG_ADAM_MAX_SEGS ? n_seg - k0 : DG_ADAM_MAX_SEGS;
        DG_HIP(dg_launch_adam(segs + k0, c, groups, n_groups, device_steps != 0,
                              tickets ? static_cast<unsigned int*>(tickets) + k0 : nullptr, static_cast<hipStream_t>(stream_)));
    }
    return DG_OK;
}

// ---- fused attention forward of the frozen ViT (dg_attn.hip)
extern "C" size_t dg_attention_workspace_bytes(int32_t B, int32_t heads, int32_t N) {
    if (B < 1 || heads < 1 || N < 1 || N > (1 << 24) || (long long)B * heads > 65535) return 0;
    return up(dg_attn_workspace(B, heads, N), 256);
}

extern "C" int dg_attention_forward(const float* qkv, int32_t B, int32_t N, int32_t heads, int32_t head_dim, float scale, float* out,
                                    void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (head_dim != 64) return fail(DG_ERR_UNSUPPORTED, "dg_attention_forward: head_dim=%d (the kernel is built for 64)", head_dim);
    if (B < 1 || heads < 1 || N < 1 || N > (1 << 24))
        return fail(DG_ERR_INVALID, "dg_attention_forward: B=%d heads=%d N=%d", B, heads, N);
    if ((long long)B * heads > 65535) return fail(DG_ERR_UNSUPPORTED, "dg_attention_forward: B * heads = %lld above 65535", (long long)B * heads);
    if (!(scale == scale) || std::isinf(scale)) return fail(DG_ERR_INVALID, "dg_attention_forward: scale=%g", (double)scale);
    if (!qkv || !out || !workspace) return fail(DG_ERR_INVALID, "dg_attention_forward: null pointer");
    if (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)workspace) & 15)
        return fail(DG_ERR_INVALID, "dg_attention_forward: qkv, out and workspace must be 16-byte aligned");
    const size_t need = dg_attention_workspace_bytes(B, heads, N);
    if (workspace_bytes < need)
        return fail(DG_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed (dg_attention_workspace_bytes)", workspace_bytes, need);
    DG_HIP(dg_launch_attention(qkv, out, workspace, B, N, heads, scale, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- fused bf16 linear layers of the frozen ViT (dg_linear.hip)
extern "C" size_t dg_vit_linear_packed_bytes(int32_t K, int32_t Nout) { return dg_linear_packed_bytes(K, Nout); }

extern "C" int dg_vit_linear_pack(const float* weight, int32_t K, int32_t Nout, void* packed, dg_stream_t stream_) {
    if (!dg_linear_supported(K, Nout))
        return fail(DG_ERR_UNSUPPORTED, "dg_vit_linear_pack: K=%d Nout=%d (multiples of 64 up to 3072)", K, Nout);
    if (!weight || !packed) return fail(DG_ERR_INVALID, "dg_vit_linear_pack: null pointer");
    if (((uintptr_t)weight | (uintptr_t)packed) & 15) return fail(DG_ERR_INVALID, "dg_vit_linear_pack: weight and packed must be 16-byte aligned");
    DG_HIP(dg_launch_linear_pack(weight, K, Nout, packed, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_vit_linear_forward(const void* x, const float* gamma, const float* beta, float eps, const void* packed, const float* bias,
                                     const float* residual, void* out, int32_t M, int32_t K, int32_t Nout, int32_t flags,
                                     dg_stream_t stream_) {
    if (!dg_linear_supported(K, Nout))
        return fail(DG_ERR_UNSUPPORTED, "dg_vit_linear_forward: K=%d Nout=%d (multiples of 64 up to 3072)", K, Nout);
    if (flags & ~(DG_LIN_LAYERNORM | DG_LIN_GELU | DG_LIN_IN_BF16 | DG_LIN_OUT_BF16))
        return fail(DG_ERR_INVALID, "dg_vit_linear_forward: unknown flags 0x%x", flags);
    if (M < 1 || M > (1 << 24)) return fail(DG_ERR_INVALID, "dg_vit_linear_forward: M=%d", M);
    if (!x || !packed || !out) return fail(DG_ERR_INVALID, "dg_vit_linear_forward: null pointer");
    if (flags & DG_LIN_LAYERNORM) {
        if (K > 768) return fail(DG_ERR_UNSUPPORTED, "dg_vit_linear_forward: LayerNorm prologue with K=%d (up to 768)", K);
        if (flags & DG_LIN_IN_BF16) return fail(DG_ERR_INVALID, "dg_vit_linear_forward: the LayerNorm prologue reads fp32 rows");
        if (!gamma || !beta) return fail(DG_ERR_INVALID, "dg_vit_linear_forward: the LayerNorm prologue needs gamma and beta");
        if (!(eps >= 0.f) || std::isinf(eps)) return fail(DG_ERR_INVALID, "dg_vit_linear_forward: eps=%g", (double)eps);
    } else {
        gamma = beta = nullptr;
    }
    if (residual && (flags & DG_LIN_OUT_BF16)) return fail(DG_ERR_INVALID, "dg_vit_linear_forward: the residual stream is fp32, not a bf16 output");
    if (x == out) return fail(DG_ERR_INVALID, "dg_vit_linear_forward: out may alias residual, not x");
    if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)packed | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)out) & 15)
        return fail(DG_ERR_INVALID, "dg_vit_linear_forward: every pointer must be 16-byte aligned");
    DG_HIP(dg_launch_linear(x, gamma, beta, eps, packed, bias, residual, out, M, K, Nout, flags, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- the fused depth encoder (dg_depth_enc.hip)
static int depthenc_check(const char* who, int32_t B, int32_t C, int32_t h, int32_t w, int32_t depth_h, int32_t depth_w) {
    if (B < 1 || h < 1 || w < 1) return fail(DG_ERR_INVALID, "%s: B=%d, feature grid %dx%d must be positive", who, B, h, w);
    if (C < 64 || C > DG_DE_MAX_C || C % 64)
        return fail(DG_ERR_UNSUPPORTED, "%s: C=%d: the last convolution's width must be a multiple of 64 up to %d", who, C, DG_DE_MAX_C);
    if ((long long)B * h * w > DG_DE_MAX_POS) return fail(DG_ERR_UNSUPPORTED, "%s: B h w = %lld positions above %d", who, (long long)B * h * w, DG_DE_MAX_POS);
    if (depth_h != 8 * h || depth_w != 8 * w)
        return fail(DG_ERR_INVALID, "%s: the depth map is %dx%d, the three-stage stack shrinks by 8: a %dx%d grid needs %dx%d", who, depth_h,
                    depth_w, h, w, 8 * h, 8 * w);
    return DG_OK;
}

static DgDepthEncArgs depthenc_args(void* workspace, bool backward, const float* depth, const float* w1, const float* b1, const float* g1,
                                    const float* be1, const float* w2, const float* b2, const float* g2, const float* be2, const float* w3,
                                    const float* b3, int32_t B, int32_t C, int32_t h, int32_t w) {
    DgDepthEncArgs A;
    memset(&A, 0, sizeof(A));
    const DgDepthWs ws = dg_depth_ws(B, C, h, w, backward);
    char* base = static_cast<char*>(workspace);
    A.depth = depth; A.w1 = w1; A.b1 = b1; A.g1 = g1; A.be1 = be1; A.w2 = w2; A.b2 = b2; A.g2 = g2; A.be2 = be2; A.w3 = w3; A.b3 = b3;
    A.pack_w2 = base + ws.pack_w2; A.pack_w3 = base + ws.pack_w3; A.pack_w2t = base + ws.pack_w2t; A.pack_w3t = base + ws.pack_w3t;
    A.x2t = base + ws.x2t; A.da2t = base + ws.da2t;
    A.part_small = reinterpret_cast<float*>(base + ws.part_small); A.part_w2 = reinterpret_cast<float*>(base + ws.part_w2);
    A.part_w3 = reinterpret_cast<float*>(base + ws.part_w3);
    A.B = B; A.C = C; A.h = h; A.w = w; A.P = h * w; A.N = B * h * w;
    A.tiles = ws.tiles; A.blocks_act = ws.blocks_act; A.splits_w2 = ws.splits_w2; A.splits_w3 = ws.splits_w3;
    return A;
}

extern "C" size_t dg_depthenc_workspace_bytes(int32_t B, int32_t C, int32_t h, int32_t w, int32_t backward) {
    if (!dg_depthenc_supported(B, C, h, w)) return 0;
    return dg_depth_ws(B, C, h, w, backward != 0).total;
}

extern "C" int dg_depthenc_forward(const float* depth, const float* w1, const float* b1, const float* gamma1, const float* beta1,
                                   const float* w2, const float* b2, const float* gamma2, const float* beta2, const float* w3,
                                   const float* b3, const float* residual, int32_t residual_h, int32_t residual_w, int32_t B, int32_t C,
                                   int32_t h, int32_t w, int32_t depth_h, int32_t depth_w, float* out, void* workspace,
                                   size_t workspace_bytes, dg_stream_t stream_) {
    if (int rc = depthenc_check(__func__, B, C, h, w, depth_h, depth_w)) return rc;
    if (residual && (residual_h != h || residual_w != w))
        return fail(DG_ERR_INVALID, "dg_depthenc_forward: the residual's grid is %dx%d, the encoder's result %dx%d: pass a (B, C, h, w) map", residual_h,
                    residual_w, h, w);
    if (!depth || !w1 || !b1 || !gamma1 || !beta1 || !w2 || !b2 || !gamma2 || !beta2 || !w3 || !b3 || !out || !workspace)
        return fail(DG_ERR_INVALID, "dg_depthenc_forward: null pointer");
    if (int rc = check_aligned(__func__, {depth, w1, b1, gamma1, beta1, w2, b2, gamma2, beta2, w3, b3, residual, out}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_depth_ws(B, C, h, w, false).total, "dg_depthenc_workspace_bytes")) return rc;
    DgDepthEncArgs A = depthenc_args(workspace, false, depth, w1, b1, gamma1, beta1, w2, b2, gamma2, beta2, w3, b3, B, C, h, w);
    A.residual = residual; A.out = out;
    DG_HIP(dg_launch_depthenc_forward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_depthenc_backward(const float* depth, const float* w1, const float* b1, const float* gamma1, const float* beta1,
                                    const float* w2, const float* b2, const float* gamma2, const float* beta2, const float* w3,
                                    const float* b3, const float* grad_out, int32_t B, int32_t C, int32_t h, int32_t w, int32_t depth_h,
                                    int32_t depth_w, float* grad_w1, float* grad_b1, float* grad_gamma1, float* grad_beta1, float* grad_w2,
                                    float* grad_b2, float* grad_gamma2, float* grad_beta2, float* grad_w3, float* grad_b3, void* workspace,
                                    size_t workspace_bytes, dg_stream_t stream_) {
    if (int rc = depthenc_check(__func__, B, C, h, w, depth_h, depth_w)) return rc;
    if (!depth || !w1 || !b1 || !gamma1 || !beta1 || !w2 || !b2 || !gamma2 || !beta2 || !w3 || !b3 || !grad_out || !workspace)
        return fail(DG_ERR_INVALID, "dg_depthenc_backward: null pointer");
    if (!grad_w1 || !grad_b1 || !grad_gamma1 || !grad_beta1 || !grad_w2 || !grad_b2 || !grad_gamma2 || !grad_beta2 || !grad_w3 || !grad_b3)
        return fail(DG_ERR_INVALID, "dg_depthenc_backward: null gradient pointer (all ten are written)");
    if (int rc = check_aligned(__func__, {depth, w1, b1, gamma1, beta1, w2, b2, gamma2, beta2, w3, b3, grad_out, grad_w1, grad_b1, grad_gamma1,
                                          grad_beta1, grad_w2, grad_b2, grad_gamma2, grad_beta2, grad_w3, grad_b3}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_depth_ws(B, C, h, w, true).total, "dg_depthenc_workspace_bytes")) return rc;
    DgDepthEncArgs A = depthenc_args(workspace, true, depth, w1, b1, gamma1, beta1, w2, b2, gamma2, beta2, w3, b3, B, C, h, w);
    A.grad_out = grad_out;
    A.d_w1 = grad_w1; A.d_b1 = grad_b1; A.d_g1 = grad_gamma1; A.d_be1 = grad_beta1; A.d_w2 = grad_w2; A.d_b2 = grad_b2; A.d_g2 = grad_gamma2;
    A.d_be2 = grad_beta2; A.d_w3 = grad_w3; A.d_b3 = grad_b3;
    DG_HIP(dg_launch_depthenc_backward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- fused cross-attention of the depth guidance (dg_xattn.hip)
static bool xattn_supported(int32_t B, int32_t heads, int32_t Nq, int32_t Nk) {
    return B >= 1 && heads >= 1 && Nq >= 1 && Nk >= 1 && Nq <= (1 << 24) && Nk <= (1 << 24) && (long long)B * heads <= 65535;
}

// what every entry refuses before it looks at a pointer
static int xattn_check(const char* who, int32_t B, int32_t heads, int32_t Nq, int32_t Nk, int32_t head_dim, float scale, float p) {
    if (head_dim != DG_XATTN_HD) return fail(DG_ERR_UNSUPPORTED, "%s: head_dim=%d (the kernels are built for %d)", who, head_dim, DG_XATTN_HD);
    if (B < 1 || heads < 1 || Nq < 1 || Nk < 1 || Nq > (1 << 24) || Nk > (1 << 24))
        return fail(DG_ERR_INVALID, "%s: B=%d heads=%d Nq=%d Nk=%d (all >= 1, Nq and Nk up to 2^24)", who, B, heads, Nq, Nk);
    if ((long long)B * heads > 65535) return fail(DG_ERR_UNSUPPORTED, "%s: B * heads = %lld above 65535", who, (long long)B * heads);
    if (!(p >= 0.f && p < 1.f)) return fail(DG_ERR_INVALID, "%s: dropout p=%g outside [0, 1)", who, (double)p);
    if (!(scale == scale) || std::isinf(scale)) return fail(DG_ERR_INVALID, "%s: scale=%g", who, (double)scale);
    return DG_OK;
}

static uint32_t xattn_threshold(float p) {            // keep iff word >= floor(p 2^32); 0 exactly when p == 0 for every p this library meets
    const double t = std::floor((double)p * 4294967296.0);
    return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}

extern "C" size_t dg_xattn_workspace_bytes(int32_t B, int32_t heads, int32_t Nq, int32_t Nk, int32_t backward) {
    if (!xattn_supported(B, heads, Nq, Nk)) return 0;
    return dg_xattn_ws(B, heads, Nq, Nk, backward != 0).total;
}

extern "C" int dg_xattn_forward(const float* q, const float* k, const float* v, int32_t B, int32_t heads, int32_t Nq, int32_t Nk,
                                int32_t head_dim, float scale, float p, uint64_t seed, float* out, float* lse, void* workspace,
                                size_t workspace_bytes, dg_stream_t stream_) {
    if (int rc = xattn_check(__func__, B, heads, Nq, Nk, head_dim, scale, p)) return rc;
    if (!q || !k || !v || !out || !workspace) return fail(DG_ERR_INVALID, "dg_xattn_forward: null pointer");
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)workspace) & 15)
        return fail(DG_ERR_INVALID, "dg_xattn_forward: q, k, v, out and workspace must be 16-byte aligned");
    if ((uintptr_t)lse & 3) return fail(DG_ERR_INVALID, "dg_xattn_forward: lse must be 4-byte aligned");
    if (int rc = check_workspace(__func__, workspace_bytes, dg_xattn_ws(B, heads, Nq, Nk, false).total, "dg_xattn_workspace_bytes")) return rc;
    DgXattnArgs A;
    memset(&A, 0, sizeof(A));
    A.q = q; A.k = k; A.v = v; A.out_w = out; A.lse_w = lse; A.workspace = workspace;
    A.B = B; A.heads = heads; A.Nq = Nq; A.Nk = Nk; A.scale = scale; A.seed = seed;
    A.thr = xattn_threshold(p); A.inv_keep = 1.f / (1.f - p);
    DG_HIP(dg_launch_xattn_forward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_xattn_backward(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* grad_out,
                                 int32_t B, int32_t heads, int32_t Nq, int32_t Nk, int32_t head_dim, float scale, float p, uint64_t seed,
                                 float* grad_q, float* grad_k, float* grad_v, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (int rc = xattn_check(__func__, B, heads, Nq, Nk, head_dim, scale, p)) return rc;
    if (!q || !k || !v || !out || !lse || !grad_out || !workspace) return fail(DG_ERR_INVALID, "dg_xattn_backward: null pointer");
    if (!grad_k != !grad_v) return fail(DG_ERR_INVALID, "dg_xattn_backward: grad_k and grad_v come from one kernel: give both or neither");
    if (!grad_q && !grad_k) return fail(DG_ERR_INVALID, "dg_xattn_backward: no gradient asked for");
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)grad_out | (uintptr_t)grad_q | (uintptr_t)grad_k |
         (uintptr_t)grad_v | (uintptr_t)workspace) & 15)
        return fail(DG_ERR_INVALID, "dg_xattn_backward: the tensors, the gradients and workspace must be 16-byte aligned");
    if ((uintptr_t)lse & 3) return fail(DG_ERR_INVALID, "dg_xattn_backward: lse must be 4-byte aligned");
    if (int rc = check_workspace(__func__, workspace_bytes, dg_xattn_ws(B, heads, Nq, Nk, true).total, "dg_xattn_workspace_bytes")) return rc;
    DgXattnArgs A;
    memset(&A, 0, sizeof(A));
    A.q = q; A.k = k; A.v = v; A.out = out; A.lse = lse; A.d_out = grad_out; A.d_q = grad_q; A.d_k = grad_k; A.d_v = grad_v;
    A.workspace = workspace;
    A.B = B; A.heads = heads; A.Nq = Nq; A.Nk = Nk; A.scale = scale; A.seed = seed;
    A.thr = xattn_threshold(p); A.inv_keep = 1.f / (1.f - p);
    DG_HIP(dg_launch_xattn_backward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_xattn_keep_mask(uint64_t seed, int32_t B, int32_t heads, int32_t Nq, int32_t Nk, float p, uint8_t* out,
                                  dg_stream_t stream_) {
    if (int rc = xattn_check(__func__, B, heads, Nq, Nk, DG_XATTN_HD, 1.f, p)) return rc;
    if (!out) return fail(DG_ERR_INVALID, "dg_xattn_keep_mask: null pointer");
    DG_HIP(dg_launch_xattn_mask(out, B, heads, Nq, Nk, seed, xattn_threshold(p), static_cast<hipStream_t>(stream_)));
    return DG_OK;
}
