// C ABI of the gfx950 DepthG library (include/depthg_corr.h): the training step's auxiliary loss terms - contrastive CRF,
// augmentation-alignment, reconstruction.  Host-side only: argument checks and kernel launches on the caller's stream.
// Every entry point has one shape: the term's dimension check, null pointers, check_aligned, check_workspace, the term's argument
// block from its *_args function, the direction's own fields, the launch.
#include "dg_api.h"
#include "dg_loss_args.h"

// ---- the contrastive CRF loss term (dg_crf_loss.hip)
static int crfl_check(const char* who, int32_t B, int32_t D, int32_t h, int32_t w, int32_t size, int32_t n) {
    if (B < 1 || h < 1 || w < 1) return fail(DG_ERR_INVALID, "%s: B=%d, code map %dx%d must be positive", who, B, h, w);
    if (D < 1 || D > DG_CRFL_MAX_D) return fail(DG_ERR_INVALID, "%s: D=%d outside 1..%d", who, D, DG_CRFL_MAX_D);
    if (n < 1 || n > DG_CRFL_MAX_N) return fail(DG_ERR_INVALID, "%s: n=%d outside 1..%d", who, n, DG_CRFL_MAX_N);
    if (size < 1 || size > DG_CRFL_MAX_SIZE) return fail(DG_ERR_INVALID, "%s: size=%d outside 1..%d", who, size, DG_CRFL_MAX_SIZE);
    if (B > 65535 || h > DG_CRFL_MAX_SIDE || w > DG_CRFL_MAX_SIDE)
        return fail(DG_ERR_UNSUPPORTED, "%s: B=%d above 65535 or a code map side above %d (%dx%d)", who, B, DG_CRFL_MAX_SIDE, h, w);
    return DG_OK;
}

// what both directions read: the workspace sections, the coordinates, the sizes
static DgCrflArgs crfl_args(void* workspace, const int32_t* coords, int32_t B, int32_t D, int32_t h, int32_t w, int32_t size, int32_t n) {
    DgCrflArgs A;
    memset(&A, 0, sizeof(A));
    const DgCrflWs ws = dg_crfl_ws(B, D, n);
    A.coords = coords;
    A.S = dg_ws_at<float>(workspace, ws.S); A.G = dg_ws_at<float>(workspace, ws.G); A.g4 = dg_ws_at<float>(workspace, ws.g4);
    A.nrm = dg_ws_at<float>(workspace, ws.nrm); A.q = dg_ws_at<double>(workspace, ws.q); A.part = dg_ws_at<double>(workspace, ws.part);
    A.B = B; A.D = D; A.Dp = (D + 3) / 4 * 4; A.h = h; A.w = w; A.size = size; A.n = n;
    return A;
}

extern "C" size_t dg_crfloss_workspace_bytes(int32_t B, int32_t D, int32_t n) {
    if (B < 1 || B > 65535 || D < 1 || D > DG_CRFL_MAX_D || n < 1 || n > DG_CRFL_MAX_N) return 0;
    return dg_crfl_ws(B, D, n).total;
}

extern "C" int dg_crfloss_forward(const float* code, const float* img, int32_t B, int32_t D, int32_t h, int32_t w, int32_t H, int32_t W,
                                  int32_t size, const int32_t* coords, int32_t n, float alpha, float beta, float gamma, float w1,
                                  float w2, float shift, void* workspace, size_t workspace_bytes, float* out_loss, dg_stream_t stream_) {
    if (int rc = crfl_check(__func__, B, D, h, w, size, n)) return rc;
    if (H < 1 || W < 1) return fail(DG_ERR_INVALID, "dg_crfloss_forward: image %dx%d must be positive", H, W);
    if (H > DG_CRFL_MAX_SIDE || W > DG_CRFL_MAX_SIDE) return fail(DG_ERR_UNSUPPORTED, "dg_crfloss_forward: image %dx%d above %d a side", H, W, DG_CRFL_MAX_SIDE);
    if (!(alpha > 0.f) || !(beta > 0.f) || !(gamma > 0.f) || std::isinf(alpha) || std::isinf(beta) || std::isinf(gamma))
        return fail(DG_ERR_INVALID, "dg_crfloss_forward: alpha=%g, beta=%g, gamma=%g must be positive and finite", (double)alpha, (double)beta, (double)gamma);
    if (!std::isfinite(w1) || !std::isfinite(w2) || !std::isfinite(shift))
        return fail(DG_ERR_INVALID, "dg_crfloss_forward: w1=%g, w2=%g, shift=%g must be finite", (double)w1, (double)w2, (double)shift);
    if (!code || !img || !coords || !workspace || !out_loss) return fail(DG_ERR_INVALID, "dg_crfloss_forward: null pointer");
    if (int rc = check_aligned(__func__, {code, img, coords, out_loss}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_crfl_ws(B, D, n).total, "dg_crfloss_workspace_bytes")) return rc;
    DgCrflArgs A = crfl_args(workspace, coords, B, D, h, w, size, n);
    A.code = code; A.img = img; A.loss = out_loss; A.H = H; A.W = W;
    A.a2 = 2.f * alpha; A.b2 = 2.f * beta; A.g2 = 2.f * gamma; A.w1 = w1; A.w2 = w2; A.shift = shift;
    DG_HIP(dg_launch_crfl_forward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_crfloss_backward(const void* workspace, size_t workspace_bytes, const int32_t* coords, int32_t B, int32_t D, int32_t h,
                                   int32_t w, int32_t size, int32_t n, const float* grad_out, float* grad_code, dg_stream_t stream_) {
    if (int rc = crfl_check(__func__, B, D, h, w, size, n)) return rc;
    if (!workspace || !coords || !grad_out || !grad_code) return fail(DG_ERR_INVALID, "dg_crfloss_backward: null pointer");
    if (int rc = check_aligned(__func__, {coords, grad_out, grad_code}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_crfl_ws(B, D, n).total, "dg_crfloss_workspace_bytes")) return rc;
    DgCrflArgs A = crfl_args(const_cast<void*>(workspace), coords, B, D, h, w, size, n);
    A.grad_out = grad_out; A.grad_code = grad_code;
    DG_HIP(dg_launch_crfl_backward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- the augmentation-alignment loss term (dg_aug.hip)
static int aug_check(const char* who, int32_t B, int32_t D, int32_t h, int32_t w, int32_t n) {
    if (B < 1 || D < 1 || h < 1 || w < 1 || n < 1)
        return fail(DG_ERR_INVALID, "%s: B=%d, D=%d, code map %dx%d and n=%d must be positive", who, B, D, h, w, n);
    if (B > 65535 || D > (1 << 20)) return fail(DG_ERR_UNSUPPORTED, "%s: B=%d above 65535 or D=%d above 2^20", who, B, D);
    if (!dg_aug_fits(h, w, n))
        return fail(DG_ERR_UNSUPPORTED, "%s: code map %dx%d under %dx%d positions: the inverse tap records index positions with 16 bits "
                    "(n <= 255) and are built in LDS (8 h w + 24 n^2 + 4 = %zu bytes, %d at most)", who, h, w, n, n,
                    h <= 16384 && w <= 16384 && n <= 16384 ? dg_aug_taps_lds(h * w, n * n) : (size_t)0, DG_AUG_MAX_LDS);
    return DG_OK;
}

// what both directions read: the two maps, the workspace sections, the sizes
static DgAugArgs aug_args(const float* code, const float* code_aug, void* workspace, int32_t B, int32_t D, int32_t h, int32_t w, int32_t n) {
    DgAugArgs A;
    memset(&A, 0, sizeof(A));
    const DgAugWs ws = dg_aug_ws(B, D, h, w, n);
    A.code = code; A.code_aug = code_aug;
    A.ds = dg_ws_at<float>(workspace, ws.ds); A.nu = dg_ws_at<float>(workspace, ws.nu); A.nv = dg_ws_at<float>(workspace, ws.nv);
    A.s = dg_ws_at<float>(workspace, ws.s); A.part = dg_ws_at<double>(workspace, ws.part); A.du = dg_ws_at<float>(workspace, ws.du);
    A.taps = dg_ws_at<char>(workspace, ws.taps); A.dsd = dg_ws_at<double>(workspace, ws.dsd);
    A.B = B; A.D = D; A.h = h; A.w = w; A.n = n;
    return A;
}

extern "C" size_t dg_augalign_workspace_bytes(int32_t B, int32_t D, int32_t h, int32_t w, int32_t n) {
    if (B < 1 || B > 65535 || D < 1 || D > (1 << 20) || !dg_aug_fits(h, w, n)) return 0;
    return dg_aug_ws(B, D, h, w, n).total;
}

extern "C" int dg_augalign_forward(const float* code, const float* code_aug, const float* coord_aug, int32_t B, int32_t D, int32_t h,
                                   int32_t w, int32_t n, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* out_loss,
                                   dg_stream_t stream_) {
    if (int rc = aug_check(__func__, B, D, h, w, n)) return rc;
    if (H < 1 || W < 1) return fail(DG_ERR_INVALID, "dg_augalign_forward: coordinate map %dx%d must be positive", H, W);
    if (H > DG_AUG_MAX_SIDE || W > DG_AUG_MAX_SIDE)
        return fail(DG_ERR_UNSUPPORTED, "dg_augalign_forward: coordinate map %dx%d above %d a side", H, W, DG_AUG_MAX_SIDE);
    if (!code || !code_aug || !coord_aug || !workspace || !out_loss) return fail(DG_ERR_INVALID, "dg_augalign_forward: null pointer");
    if (int rc = check_aligned(__func__, {code, code_aug, coord_aug, out_loss}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_aug_ws(B, D, h, w, n).total, "dg_augalign_workspace_bytes")) return rc;
    DgAugArgs A = aug_args(code, code_aug, workspace, B, D, h, w, n);
    A.coord_aug = coord_aug; A.loss = out_loss; A.H = H; A.W = W;
    DG_HIP(dg_launch_aug_forward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_augalign_backward(const float* code, const float* code_aug, void* workspace, size_t workspace_bytes, int32_t B,
                                    int32_t D, int32_t h, int32_t w, int32_t n, const float* grad_out, float* grad_code,
                                    float* grad_code_aug, dg_stream_t stream_) {
    if (int rc = aug_check(__func__, B, D, h, w, n)) return rc;
    if (!code || !code_aug || !workspace || !grad_out || !grad_code || !grad_code_aug)
        return fail(DG_ERR_INVALID, "dg_augalign_backward: null pointer");
    if (int rc = check_aligned(__func__, {code, code_aug, grad_out, grad_code, grad_code_aug}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_aug_ws(B, D, h, w, n).total, "dg_augalign_workspace_bytes")) return rc;
    DgAugArgs A = aug_args(code, code_aug, workspace, B, D, h, w, n);
    A.grad_out = grad_out; A.grad_code = grad_code; A.grad_code_aug = grad_code_aug;
    DG_HIP(dg_launch_aug_backward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- the reconstruction loss term (dg_rec_loss.hip)
static int rec_check(const char* who, int32_t B, int32_t D, int32_t C, int32_t h, int32_t w) {
    if (B < 1 || D < 1 || C < 1 || h < 1 || w < 1)
        return fail(DG_ERR_INVALID, "%s: B=%d, D=%d, C=%d and the map %dx%d must be positive", who, B, D, C, h, w);
    if (D > DG_REC_MAX_D) return fail(DG_ERR_UNSUPPORTED, "%s: D=%d above %d (the head's limit)", who, D, DG_REC_MAX_D);
    if (!dg_rec_fits(B, D, C, h, w))
        return fail(DG_ERR_UNSUPPORTED, "%s: B=%d, D=%d, C=%d, map %dx%d: a tensor of 2^31 elements or more", who, B, D, C, h, w);
    return DG_OK;
}

// what both directions read: the maps, the decoder, the Dropout2d flags, the workspace sections, the sizes
static DgRecArgs rec_args(const float* code, const float* feats, const float* weight, const float* bias, const float* keep, float scale,
                          void* workspace, int32_t B, int32_t D, int32_t C, int32_t h, int32_t w) {
    DgRecArgs A;
    memset(&A, 0, sizeof(A));
    const DgRecWs ws = dg_rec_ws(B, D, C, h, w);
    A.code = code; A.feats = feats; A.weight = weight; A.bias = bias; A.keep = keep; A.scale = scale;
    A.ny = dg_ws_at<float>(workspace, ws.ny); A.nf = dg_ws_at<float>(workspace, ws.nf); A.s = dg_ws_at<float>(workspace, ws.s);
    A.part = dg_ws_at<double>(workspace, ws.part); A.wpart = dg_ws_at<float>(workspace, ws.wpart); A.bpart = dg_ws_at<float>(workspace, ws.bpart);
    A.B = B; A.D = D; A.C = C; A.P = h * w; A.tiles_per_img = dg_rec_tiles_per_img(h, w); A.splits = dg_rec_splits(B, C, h, w);
    A.inv_n = 1.0 / ((double)B * (double)h * (double)w);
    return A;
}

extern "C" size_t dg_recloss_workspace_bytes(int32_t B, int32_t D, int32_t C, int32_t h, int32_t w) {
    if (!dg_rec_fits(B, D, C, h, w)) return 0;
    return dg_rec_ws(B, D, C, h, w).total;
}

extern "C" int dg_recloss_forward(const float* code, const float* feats, const float* weight, const float* bias, const float* keep,
                                  float scale, int32_t B, int32_t D, int32_t C, int32_t h, int32_t w, void* workspace,
                                  size_t workspace_bytes, float* out_loss, dg_stream_t stream_) {
    if (int rc = rec_check(__func__, B, D, C, h, w)) return rc;
    if (!code || !feats || !weight || !bias || !workspace || !out_loss) return fail(DG_ERR_INVALID, "dg_recloss_forward: null pointer");
    if (keep && !(scale > 0.f && !std::isinf(scale))) return fail(DG_ERR_INVALID, "dg_recloss_forward: keep scale=%g must be positive and finite", (double)scale);
    if (int rc = check_aligned(__func__, {code, feats, weight, bias, keep, out_loss}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_rec_ws(B, D, C, h, w).total, "dg_recloss_workspace_bytes")) return rc;
    DgRecArgs A = rec_args(code, feats, weight, bias, keep, scale, workspace, B, D, C, h, w);
    A.loss = out_loss;
    DG_HIP(dg_launch_rec_forward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_recloss_backward(const float* code, const float* feats, const float* weight, const float* bias, const float* keep,
                                   float scale, void* workspace, size_t workspace_bytes, int32_t B, int32_t D, int32_t C, int32_t h,
                                   int32_t w, const float* grad_out, float* grad_code, float* grad_weight, float* grad_bias,
                                   dg_stream_t stream_) {
    if (int rc = rec_check(__func__, B, D, C, h, w)) return rc;
    if (!code || !feats || !weight || !bias || !workspace || !grad_out || !grad_code || !grad_weight || !grad_bias)
        return fail(DG_ERR_INVALID, "dg_recloss_backward: null pointer");
    if (keep && !(scale > 0.f && !std::isinf(scale))) return fail(DG_ERR_INVALID, "dg_recloss_backward: keep scale=%g must be positive and finite", (double)scale);
    if (int rc = check_aligned(__func__, {code, feats, weight, bias, keep, grad_out, grad_code, grad_weight, grad_bias}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_rec_ws(B, D, C, h, w).total, "dg_recloss_workspace_bytes")) return rc;
    DgRecArgs A = rec_args(code, feats, weight, bias, keep, scale, workspace, B, D, C, h, w);
    A.grad_out = grad_out; A.grad_code = grad_code; A.grad_weight = grad_weight; A.grad_bias = grad_bias;
    DG_HIP(dg_launch_rec_backward(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// the backward with d feats: everything in one call; grad_code, grad_weight and grad_bias are given or null together
extern "C" int dg_rec_feats_backward(const float* code, const float* feats, const float* weight, const float* bias, const float* keep,
                                     float scale, void* workspace, size_t workspace_bytes, int32_t B, int32_t D, int32_t C, int32_t h,
                                     int32_t w, const float* grad_out, float* grad_code, float* grad_weight, float* grad_bias,
                                     float* grad_feats, dg_stream_t stream_) {
    if (int rc = rec_check(__func__, B, D, C, h, w)) return rc;
    if (!code || !feats || !weight || !bias || !workspace || !grad_out || !grad_feats)
        return fail(DG_ERR_INVALID, "dg_rec_feats_backward: null pointer");
    if ((grad_code != nullptr) != (grad_weight != nullptr) || (grad_code != nullptr) != (grad_bias != nullptr))
        return fail(DG_ERR_INVALID, "dg_rec_feats_backward: grad_code, grad_weight and grad_bias are given together or null together");
    if (keep && !(scale > 0.f && !std::isinf(scale))) return fail(DG_ERR_INVALID, "dg_rec_feats_backward: keep scale=%g must be positive and finite", (double)scale);
    if (int rc = check_aligned(__func__, {code, feats, weight, bias, keep, grad_out, grad_code, grad_weight, grad_bias, grad_feats}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_rec_ws(B, D, C, h, w).total, "dg_recloss_workspace_bytes")) return rc;
    DgRecArgs A = rec_args(code, feats, weight, bias, keep, scale, workspace, B, D, C, h, w);
    A.grad_out = grad_out; A.grad_code = grad_code; A.grad_weight = grad_weight; A.grad_bias = grad_bias; A.grad_feats = grad_feats;
    DG_HIP(dg_launch_rec_backward_feats(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}
