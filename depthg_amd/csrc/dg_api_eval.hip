// C ABI of the gfx950 DepthG library (include/depthg_corr.h): the probes, evaluation and the dense CRF (dg_probe.hip, dg_eval.hip,
// dg_seg_labels.hip, dg_crf.hip, dg_metrics.hip).  Host-side only: argument checks and kernel launches on the caller's stream.
#include "dg_api.h"
#include "dg_eval_args.h"
#include "dg_head_args.h"     // the probes (dg_probe.hip, dg_probe_step.hip)
#include "dg_aux_args.h"      // dg_launch_confusion (dg_metrics.hip)

extern "C" int dg_confusion_update(const int64_t* preds, const int64_t* target, int64_t count, int32_t n_classes,
                                   int32_t extra_clusters, int64_t* stats, dg_stream_t stream_) {
    if (count < 0 || n_classes < 1 || extra_clusters < 0) return fail(DG_ERR_INVALID, "bad confusion-matrix dimensions");
    if (count == 0) return DG_OK;
    if (!preds || !target || !stats) return fail(DG_ERR_INVALID, "null pointer");
    if ((long long)n_classes * (n_classes + extra_clusters) > (1 << 24)) return fail(DG_ERR_UNSUPPORTED, "confusion matrix too large");
    DG_HIP(dg_launch_confusion(reinterpret_cast<const long long*>(preds), reinterpret_cast<const long long*>(target), count,
                               n_classes, n_classes + extra_clusters, reinterpret_cast<unsigned long long*>(stats),
                               static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_cluster_lookup_forward(const float* x, const float* clusters, float alpha, int32_t B, int32_t D, int32_t n, int32_t P,
                                         float* inner, float* probs, float* logp, float* loss, float* scratch, dg_stream_t stream_) {
    if (B < 1 || D < 1 || n < 1 || P < 1) return fail(DG_ERR_INVALID, "bad cluster-lookup dimensions");
    if (D > 128 || (size_t)n * (D + 1) > 16000) return fail(DG_ERR_UNSUPPORTED, "cluster lookup needs D <= 128 and n * (D + 1) <= 16000");
    if (!x || !clusters || !inner || !loss || !scratch) return fail(DG_ERR_INVALID, "null pointer");
    DgClusterArgs a{x, clusters, alpha, inner, probs, logp, scratch, B, D, n, P};
    DG_HIP(dg_launch_cluster_fwd(a, loss, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_cluster_lookup_backward(const float* x, const float* clusters, const float* inner, float alpha, const float* grad_loss,
                                          int32_t B, int32_t D, int32_t n, int32_t P, float* grad_clusters, float* grad_x, float* scratch,
                                          dg_stream_t stream_) {
    if (B < 1 || D < 1 || n < 1 || P < 1) return fail(DG_ERR_INVALID, "bad cluster-lookup dimensions");
    if (D > 128 || (size_t)n * (D + 1) > 16000 || (size_t)(n + D) * 65 * 4 > 160 * 1024) return fail(DG_ERR_UNSUPPORTED, "cluster lookup needs D <= 128 and n * (D + 1) <= 16000");
    if (!x || !clusters || !inner || !grad_loss || !grad_clusters || !scratch) return fail(DG_ERR_INVALID, "null pointer");
    DgClusterBwdArgs a{x, clusters, inner, grad_loss, alpha, scratch, grad_x, scratch + (size_t)B * n * P, grad_clusters, B, D, n, P};
    DG_HIP(dg_launch_cluster_bwd(a, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

static int probe_check(int32_t B, int32_t n, int32_t h, int32_t w, int32_t H, int32_t W) {
    if (B < 1 || n < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail(DG_ERR_INVALID, "bad probe dimensions");
    if (n * w > 2048 || (size_t)(2 * n * w + (size_t)n * W) * 4 > 150 * 1024) return fail(DG_ERR_UNSUPPORTED, "probe loss needs n*w <= 2048 and n*(2w+W) floats of LDS");
    return DG_OK;
}
extern "C" int dg_probe_ce_forward(const float* logits, const int64_t* label, int32_t B, int32_t n, int32_t h, int32_t w, int32_t H,
                                   int32_t W, float* out3, float* scratch, dg_stream_t stream_) {
    if (int rc = probe_check(B, n, h, w, H, W)) return rc;
    if (!logits || !label || !out3 || !scratch) return fail(DG_ERR_INVALID, "null pointer");
    DgProbeCeArgs a{logits, label, scratch, nullptr, nullptr, nullptr, B, n, h, w, H, W};
    DG_HIP(dg_launch_probe_ce_fwd(a, out3, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}
extern "C" int dg_probe_ce_backward(const float* logits, const int64_t* label, const float* out3, const float* grad_loss, int32_t B,
                                    int32_t n, int32_t h, int32_t w, int32_t H, int32_t W, float* grad_logits, dg_stream_t stream_) {
    if (int rc = probe_check(B, n, h, w, H, W)) return rc;
    if (!logits || !label || !out3 || !grad_loss || !grad_logits) return fail(DG_ERR_INVALID, "null pointer");
    DgProbeCeArgs a{logits, label, nullptr, grad_loss, out3, grad_logits, B, n, h, w, H, W};
    DG_HIP(dg_launch_probe_ce_bwd(a, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- the fused probe step (dg_probe_step.hip): the plan refuses in front of any launch
static int probe_step_check(const char* who, int32_t B, int32_t D, int32_t n, int32_t m, int32_t h, int32_t w, int32_t H, int32_t W,
                            DgProbeStepPlan& pl) {
    if (B < 1 || D < 1 || n < 1 || m < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail(DG_ERR_INVALID, "%s: bad dimensions", who);
    if (const char* why = dg_probe_step_plan(B, D, n, m, h, w, H, W, pl))
        return fail(DG_ERR_UNSUPPORTED, "%s: %s (B=%d D=%d n_lin=%d n_clu=%d h=%d w=%d H=%d W=%d)", who, why, B, D, n, m, h, w, H, W);
    return DG_OK;
}
extern "C" size_t dg_probe_step_workspace_bytes(int32_t B, int32_t D, int32_t n_lin, int32_t n_clu, int32_t h, int32_t w, int32_t H, int32_t W) {
    DgProbeStepPlan pl;
    if (probe_step_check("probe step", B, D, n_lin, n_clu, h, w, H, W, pl)) return 0;
    return pl.floats * 4;
}
extern "C" int dg_probe_step_forward(const float* code, const int64_t* label, const float* lin_w, const float* lin_b, const float* clusters,
                                     int32_t B, int32_t D, int32_t n_lin, int32_t n_clu, int32_t h, int32_t w, int32_t H, int32_t W,
                                     float* out3, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    DgProbeStepPlan pl;
    if (int rc = probe_step_check("probe step forward", B, D, n_lin, n_clu, h, w, H, W, pl)) return rc;
    if (!code || !label || !lin_w || !clusters || !out3 || !workspace) return fail(DG_ERR_INVALID, "probe step forward: null pointer");
    if (int rc = check_aligned("probe step forward", {code, lin_w, lin_b, clusters, out3}, workspace)) return rc;
    if (reinterpret_cast<uintptr_t>(label) % 8) return fail(DG_ERR_INVALID, "probe step forward: label must be 8-byte aligned");
    if (int rc = check_workspace("probe step forward", workspace_bytes, pl.floats * 4, "dg_probe_step_workspace_bytes")) return rc;
    DgProbeStepArgs a{code, label, lin_w, lin_b, clusters, static_cast<float*>(workspace), out3, B, D, n_lin, n_clu, h, w, H, W};
    DG_HIP(dg_launch_probe_step_fwd(a, pl, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}
extern "C" int dg_probe_step_backward(const void* workspace, size_t workspace_bytes, const float* grad_linear, const float* grad_cluster,
                                      int32_t B, int32_t D, int32_t n_lin, int32_t n_clu, int32_t h, int32_t w, int32_t H, int32_t W,
                                      float* grad_w, float* grad_b, float* grad_clusters, dg_stream_t stream_) {
    DgProbeStepPlan pl;
    if (int rc = probe_step_check("probe step backward", B, D, n_lin, n_clu, h, w, H, W, pl)) return rc;
    if (!workspace || !grad_linear || !grad_cluster || !grad_w || !grad_b || !grad_clusters)
        return fail(DG_ERR_INVALID, "probe step backward: null pointer");
    if (int rc = check_aligned("probe step backward", {grad_linear, grad_cluster, grad_w, grad_b, grad_clusters}, workspace)) return rc;
    if (int rc = check_workspace("probe step backward", workspace_bytes, pl.floats * 4, "dg_probe_step_workspace_bytes")) return rc;
    DG_HIP(dg_launch_probe_step_bwd(static_cast<const float*>(workspace), pl, grad_linear, grad_cluster, D, n_lin, n_clu, grad_w, grad_b,
                                    grad_clusters, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_segment_predict(const float* code, const float* code_flip, int32_t B, int32_t D, int32_t h, int32_t w,
                                  const float* lin_w, const float* lin_b, int32_t n, const float* clusters, int32_t m,
                                  const int64_t* label, int32_t H, int32_t W, int64_t* stats_lin, int64_t* stats_clu, int32_t n_store,
                                  int64_t* preds_lin, int64_t* preds_clu, void* scratch, size_t scratch_bytes, dg_stream_t stream_) {
    if (B < 1 || D < 1 || h < 1 || w < 1 || n < 1 || m < 1 || H < 1 || W < 1 || n_store < 0)
        return fail(DG_ERR_INVALID, "bad segment-predict dimensions");
    if (D > DG_SEG_MAX_D) return fail(DG_ERR_UNSUPPORTED, "segment predict needs D <= %d (got %d)", DG_SEG_MAX_D, D);
    if (n + m > DG_SEG_MAX_K) return fail(DG_ERR_UNSUPPORTED, "segment predict needs n + m <= %d (got %d)", DG_SEG_MAX_K, n + m);
    if ((long long)w * dg_seg_kp(n, m) > DG_SEG_ROW_FLOATS)
        return fail(DG_ERR_UNSUPPORTED, "segment predict needs w * (n + m, each rounded up to 4) <= %d (w=%d)", DG_SEG_ROW_FLOATS, w);
    if ((long long)h * w > (1 << 24) || (long long)B * H * W > (1LL << 40)) return fail(DG_ERR_UNSUPPORTED, "maps too large");
    if (!code || !lin_w || !clusters || !label || !scratch) return fail(DG_ERR_INVALID, "null pointer");
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return fail(DG_ERR_INVALID, "scratch must be 16-byte aligned");
    const size_t need = (size_t)B * h * w * dg_seg_kp(n, m) * 4;
    if (scratch_bytes < need) return fail(DG_ERR_WORKSPACE, "scratch of %zu bytes, %zu needed", scratch_bytes, need);
    if (n_store > B) n_store = B;
    DgSegArgs a{code, code_flip, lin_w, lin_b, clusters, label, static_cast<float*>(scratch), stats_lin, stats_clu, preds_lin, preds_clu,
                B, D, h, w, n, m, H, W, n_store};
    DG_HIP(dg_launch_segment_predict(a, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- label-free inference (dg_seg_labels.hip)

// the remap, paint and output arguments dg_segment_labels and dg_label_paint share, checked
static int paint_check(const char* who, DgPaintArgs& p, int32_t B, int32_t H, int32_t W, int32_t m, const int32_t* remap, const float* img,
                       const float* mean, const float* std, const uint8_t* cmap, int32_t cmap_rows, int32_t alpha256, uint8_t* lab_lin,
                       uint8_t* lab_clu, uint8_t* rgb_lin, uint8_t* rgb_clu) {
    if (m > DG_SEG_MAX_LABELS) return fail(DG_ERR_UNSUPPORTED, "%s needs m <= %d: a byte holds the cluster id, 255 is \"no class\" (got %d)", who, DG_SEG_MAX_LABELS, m);
    if (!lab_lin && !lab_clu && !rgb_lin && !rgb_clu) return fail(DG_ERR_INVALID, "%s: nothing to write, the four outputs are null", who);
    p = DgPaintArgs{};
    p.remap = remap; p.lab_lin = lab_lin; p.lab_clu = lab_clu; p.rgb_lin = rgb_lin; p.rgb_clu = rgb_clu;
    p.B = B; p.H = H; p.W = W; p.m = m; p.cmap_rows = 1; p.alpha256 = 256;
    if (rgb_lin || rgb_clu) {
        if (cmap_rows < 1 || cmap_rows > DG_SEG_MAX_CMAP)
            return fail(DG_ERR_INVALID, "%s: a colour output needs 1 <= cmap_rows <= %d (got %d)", who, DG_SEG_MAX_CMAP, cmap_rows);
        if (!cmap) return fail(DG_ERR_INVALID, "%s: a colour output needs cmap", who);
        if (alpha256 < 0 || alpha256 > 256) return fail(DG_ERR_INVALID, "%s: alpha256 must lie in [0, 256] (got %d)", who, alpha256);
        if (alpha256 < 256 && (!img || !mean || !std))
            return fail(DG_ERR_INVALID, "%s: a colour output with alpha256 = %d < 256 blends with the image: img, mean and std are needed", who, alpha256);
        p.cmap = cmap; p.cmap_rows = cmap_rows; p.alpha256 = alpha256;
        if (alpha256 < 256) {
            if (reinterpret_cast<uintptr_t>(img) % 4) return fail(DG_ERR_INVALID, "%s: img must be 4-byte aligned", who);
            p.img = img;
            for (int c = 0; c < 3; ++c) {
                if (!std::isfinite(mean[c]) || !std::isfinite(std[c])) return fail(DG_ERR_INVALID, "%s: mean and std must be finite", who);
                p.mean[c] = mean[c]; p.std[c] = std[c];
            }
        }
    }
    return DG_OK;
}

extern "C" int dg_segment_labels(const float* code, const float* code_flip, int32_t B, int32_t D, int32_t h, int32_t w, const float* lin_w,
                                 const float* lin_b, int32_t n, const float* clusters, int32_t m, int32_t H, int32_t W, const int32_t* remap,
                                 const float* img, const float* mean, const float* std, const uint8_t* cmap, int32_t cmap_rows,
                                 int32_t alpha256, uint8_t* lab_lin, uint8_t* lab_clu, uint8_t* rgb_lin, uint8_t* rgb_clu, void* scratch,
                                 size_t scratch_bytes, dg_stream_t stream_) {
    if (B < 1 || D < 1 || h < 1 || w < 1 || n < 1 || m < 1 || H < 1 || W < 1) return fail(DG_ERR_INVALID, "bad segment-labels dimensions");
    if (D > DG_SEG_MAX_D) return fail(DG_ERR_UNSUPPORTED, "segment labels needs D <= %d (got %d)", DG_SEG_MAX_D, D);
    if (n > DG_SEG_MAX_LABELS)
        return fail(DG_ERR_UNSUPPORTED, "segment labels needs n <= %d: a byte holds the class id, 255 is \"no class\" (got %d)", DG_SEG_MAX_LABELS, n);
    DgPaintArgs p;
    if (int rc = paint_check("segment labels", p, B, H, W, m, remap, img, mean, std, cmap, cmap_rows, alpha256, lab_lin, lab_clu, rgb_lin, rgb_clu))
        return rc;
    if (n + m > DG_SEG_MAX_K) return fail(DG_ERR_UNSUPPORTED, "segment labels needs n + m <= %d (got %d)", DG_SEG_MAX_K, n + m);
    if ((long long)w * dg_seg_kp(n, m) > DG_SEG_ROW_FLOATS)
        return fail(DG_ERR_UNSUPPORTED, "segment labels needs w * (n + m, each rounded up to 4) <= %d (w=%d)", DG_SEG_ROW_FLOATS, w);
    if (W > (DG_SEG_STAGE_BYTES - 128) / 8) return fail(DG_ERR_UNSUPPORTED, "segment labels needs W <= %d (got %d)", (DG_SEG_STAGE_BYTES - 128) / 8, W);
    if ((long long)h * w > (1 << 24) || (long long)B * H > (1LL << 30) || (long long)B * H * W > (1LL << 40))
        return fail(DG_ERR_UNSUPPORTED, "maps too large");
    if (!code || !lin_w || !clusters || !scratch) return fail(DG_ERR_INVALID, "null pointer");
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return fail(DG_ERR_INVALID, "scratch must be 16-byte aligned");
    const size_t need = (size_t)B * h * w * dg_seg_kp(n, m) * 4;
    if (scratch_bytes < need) return fail(DG_ERR_WORKSPACE, "scratch of %zu bytes, %zu needed", scratch_bytes, need);
    DgSegArgs a{code, code_flip, lin_w, lin_b, clusters, nullptr, static_cast<float*>(scratch), nullptr, nullptr, nullptr, nullptr,
                B, D, h, w, n, m, H, W, 0};
    DG_HIP(dg_launch_segment_labels(a, p, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_label_paint(const int64_t* preds, int32_t n_groups, int32_t B, int32_t H, int32_t W, int32_t m, const int32_t* remap,
                              const float* img, const float* mean, const float* std, const uint8_t* cmap, int32_t cmap_rows,
                              int32_t alpha256, uint8_t* lab_lin, uint8_t* lab_clu, uint8_t* rgb_lin, uint8_t* rgb_clu, dg_stream_t stream_) {
    if (B < 1 || H < 1 || W < 1 || m < 1 || n_groups < 1) return fail(DG_ERR_INVALID, "bad label-paint dimensions");
    DgPaintArgs p;
    if (int rc = paint_check("label paint", p, B, H, W, m, remap, img, mean, std, cmap, cmap_rows, alpha256, lab_lin, lab_clu, rgb_lin, rgb_clu))
        return rc;
    if (n_groups < 2 && (lab_clu || rgb_clu)) return fail(DG_ERR_INVALID, "label paint: the cluster outputs read preds[1], n_groups is %d", n_groups);
    if ((long long)B * H * W > (1LL << 40)) return fail(DG_ERR_UNSUPPORTED, "maps too large");
    if (!preds) return fail(DG_ERR_INVALID, "null pointer");
    if (reinterpret_cast<uintptr_t>(preds) % 8) return fail(DG_ERR_INVALID, "preds must be 8-byte aligned");
    DG_HIP(dg_launch_label_paint(preds, n_groups, p, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- dense-CRF refinement (dg_crf.hip)

// group ends -> the per-group padded column offsets; C and Kp; false on bad ends
static bool crf_groups(const int32_t* group_ends, int32_t G, int32_t* gend, int32_t* goff, int& C, int& Kp) {
    if (!group_ends || G < 1 || G > DG_CRF_MAX_GROUPS) return false;
    int prev = 0, col = 0;
    for (int g = 0; g < G; ++g) {
        const int e = group_ends[g];
        if (e <= prev || e > 1 << 20) return false;
        gend[g] = e;
        goff[g] = col;
        col += (e - prev + 3) / 4 * 4;
        prev = e;
    }
    C = prev;
    Kp = col;
    return true;
}

extern "C" size_t dg_crf_workspace_bytes(int32_t chunk, int32_t H, int32_t W, int32_t Kp, int32_t lattices) {
    if (Kp < 4 || Kp % 4 || Kp > DG_CRF_MAX_KP) return 0;
    return dg_crf_chunk_bytes(chunk, H, W, Kp, lattices);
}

extern "C" int dg_crf_unary(const float* logits, int32_t B, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, const int32_t* group_ends,
                            int32_t n_groups, float* unary, dg_stream_t stream_) {
    if (B < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail(DG_ERR_INVALID, "bad crf-unary dimensions");
    int32_t gend[DG_CRF_MAX_GROUPS], goff[DG_CRF_MAX_GROUPS];
    int Cg = 0, Kp = 0;
    if (!crf_groups(group_ends, n_groups, gend, goff, Cg, Kp) || Cg != C)
        return fail(DG_ERR_INVALID, "group ends must rise strictly from above 0 to C=%d, at most %d groups", C, DG_CRF_MAX_GROUPS);
    if ((long long)H * W > DG_CRF_MAX_HW || (long long)h * w > DG_CRF_MAX_HW || (long long)B * C * H * W > (1LL << 40))
        return fail(DG_ERR_UNSUPPORTED, "maps too large");
    if (!logits || !unary) return fail(DG_ERR_INVALID, "null pointer");
    DG_HIP(dg_launch_crf_unary(logits, B, C, h, w, H, W, n_groups, gend, unary, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_segment_unary(const float* code, const float* code_flip, int32_t B, int32_t D, int32_t h, int32_t w, const float* lin_w,
                                const float* lin_b, int32_t n, const float* clusters, int32_t m, int32_t H, int32_t W, float alpha,
                                float* unary, void* scratch, size_t scratch_bytes, dg_stream_t stream_) {
    if (B < 1 || D < 1 || h < 1 || w < 1 || n < 1 || m < 1 || H < 1 || W < 1)
        return fail(DG_ERR_INVALID, "bad segment-unary dimensions");
    if (D > DG_SEG_MAX_D) return fail(DG_ERR_UNSUPPORTED, "segment unary needs D <= %d (got %d)", DG_SEG_MAX_D, D);
    if (n + m > DG_SEG_MAX_K) return fail(DG_ERR_UNSUPPORTED, "segment unary needs n + m <= %d (got %d)", DG_SEG_MAX_K, n + m);
    if ((long long)h * w > (1 << 24) || (long long)H * W > DG_CRF_MAX_HW || (long long)B * (n + m) * H * W > (1LL << 40))
        return fail(DG_ERR_UNSUPPORTED, "maps too large");
    if (!code || !lin_w || !clusters || !unary || !scratch) return fail(DG_ERR_INVALID, "null pointer");
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return fail(DG_ERR_INVALID, "scratch must be 16-byte aligned");
    const size_t need = (size_t)B * h * w * dg_seg_kp(n, m) * 4;
    if (scratch_bytes < need) return fail(DG_ERR_WORKSPACE, "scratch of %zu bytes, %zu needed", scratch_bytes, need);
    DgSegArgs a{code, code_flip, lin_w, lin_b, clusters, nullptr, static_cast<float*>(scratch), nullptr, nullptr, nullptr, nullptr,
                B, D, h, w, n, m, H, W, 0};
    DG_HIP(dg_launch_segment_unary(a, alpha, unary, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// the checks dg_crf_filter and dg_dense_crf share: sizes, workspace, key range
static int crf_check(DgCrfArgs& a, const float* stds_g, const float* stds_b, bool need_g, bool need_b) {
    if ((long long)a.H * a.W > DG_CRF_MAX_HW || (long long)a.H * a.W * 6 > 0x7fffffffLL)
        return fail(DG_ERR_UNSUPPORTED, "image of %dx%d pixels too large", a.H, a.W);
    if (a.Kp > DG_CRF_MAX_KP) return fail(DG_ERR_UNSUPPORTED, "crf needs <= %d channels, each group rounded up to 4 (got %d)", DG_CRF_MAX_KP, a.Kp);
    if (need_g && !dg_crf_key_plan(2, a.H, a.W, stds_g, a.kg))
        return fail(DG_ERR_UNSUPPORTED, "Gaussian lattice: the key range of %dx%d pixels at std %g does not fit 63 bits", a.H, a.W, (double)stds_g[0]);
    if (need_b && !dg_crf_key_plan(5, a.H, a.W, stds_b, a.kb))
        return fail(DG_ERR_UNSUPPORTED, "bilateral lattice: the key range of %dx%d pixels at std %g / %g does not fit 63 bits", a.H, a.W,
                    (double)stds_b[0], (double)stds_b[2]);
    if (!a.ws) return fail(DG_ERR_INVALID, "null workspace");
    if (reinterpret_cast<uintptr_t>(a.ws) % 256) return fail(DG_ERR_INVALID, "workspace must be 256-byte aligned");
    const int lats = (need_g ? DG_CRF_GAUSSIAN : 0) | (need_b ? DG_CRF_BILATERAL : 0);
    const size_t need = dg_crf_chunk_bytes(1, a.H, a.W, a.Kp, lats);
    if (!need) return fail(DG_ERR_UNSUPPORTED, "no workspace plan for %dx%d pixels at %d channels (lattice entries x channel quads >= 2^30)",
                           a.H, a.W, a.Kp);
    if (a.ws_bytes < need)
        return fail(DG_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed for one image (dg_crf_workspace_bytes)", a.ws_bytes, need);
    return DG_OK;
}

extern "C" int dg_crf_filter(const float* img, const float* values, int32_t B, int32_t C, int32_t H, int32_t W, int32_t bilateral, float sxy,
                             float srgb, float* out, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(DG_ERR_INVALID, "bad crf-filter dimensions");
    if (!(sxy > 0.f) || (bilateral && !(srgb > 0.f))) return fail(DG_ERR_INVALID, "standard deviations must be positive");
    if (!values || !out || (bilateral && !img)) return fail(DG_ERR_INVALID, "null pointer");
    DgCrfArgs a{};
    a.img = img; a.in = values; a.out = out; a.ws = workspace; a.ws_bytes = workspace_bytes;
    a.B = B; a.C = C; a.H = H; a.W = W; a.G = 1; a.Kp = (C + 3) / 4 * 4; a.gend[0] = C; a.goff[0] = 0;
    a.filter_bilateral = bilateral ? 1 : 0;
    const float sg[2] = {sxy, sxy}, sb[5] = {sxy, sxy, srgb, srgb, srgb};
    const int rc = crf_check(a, sg, sb, !bilateral, bilateral != 0);
    if (rc != DG_OK) return rc;
    DG_HIP(dg_launch_crf_filter(a, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_dense_crf(const float* img, const float* unary, int32_t B, int32_t H, int32_t W, const int32_t* group_ends, int32_t n_groups,
                            int32_t n_iter, float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, float* q,
                            int64_t* preds, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (B < 1 || H < 1 || W < 1 || n_iter < 0 || n_iter > 1000) return fail(DG_ERR_INVALID, "bad dense-crf dimensions");
    DgCrfArgs a{};
    int C = 0, Kp = 0;
    if (!crf_groups(group_ends, n_groups, a.gend, a.goff, C, Kp))
        return fail(DG_ERR_INVALID, "group ends must rise strictly from above 0, at most %d groups", DG_CRF_MAX_GROUPS);
    if (!(pos_xy_std > 0.f) || !(bi_xy_std > 0.f) || !(bi_rgb_std > 0.f)) return fail(DG_ERR_INVALID, "standard deviations must be positive");
    if (!std::isfinite(pos_w) || !std::isfinite(bi_w)) return fail(DG_ERR_INVALID, "Potts weights must be finite");
    if (!img || !unary) return fail(DG_ERR_INVALID, "null pointer");
    if (!q && !preds) return fail(DG_ERR_INVALID, "nothing to write: q and preds are both null");
    a.img = img; a.in = unary; a.out = q; a.preds = preds; a.ws = workspace; a.ws_bytes = workspace_bytes;
    a.B = B; a.C = C; a.H = H; a.W = W; a.G = n_groups; a.Kp = Kp; a.n_iter = n_iter; a.w_pos = pos_w; a.w_bi = bi_w;
    const float sg[2] = {pos_xy_std, pos_xy_std}, sb[5] = {bi_xy_std, bi_xy_std, bi_rgb_std, bi_rgb_std, bi_rgb_std};
    const int rc = crf_check(a, sg, sb, true, true);
    if (rc != DG_OK) return rc;
    DG_HIP(dg_launch_dense_crf(a, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}
