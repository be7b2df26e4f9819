// C ABI of the gfx950 DepthG library (include/depthg_corr.h): the segmentation head (dg_head.hip).  Host-side only: argument
// checks, workspace carving by the kernels' own plan (dg_head_plan), kernel launches on the caller's stream.
#include "dg_api.h"
#include "dg_head_args.h"

static int head_check(int32_t B, int32_t C, int32_t D, int32_t P) {
    if (B < 1 || C < 1 || D < 1 || P < 1) return fail(DG_ERR_INVALID, "bad head dimensions");
    if (C > 768 || (C & 7)) return fail(DG_ERR_UNSUPPORTED, "C=%d: the head needs C <= 768 and a multiple of 8", C);
    if (D > 128) return fail(DG_ERR_UNSUPPORTED, "D=%d > 128 code channels not supported", D);
    return DG_OK;
}
static size_t head_weights_bytes(int32_t C, int32_t D) {
    return DgHeadWeightLayout(C, D).elems * 2;
}
extern "C" size_t dg_head_weights_bytes(int32_t C, int32_t D) {
    if (head_check(1, C, D, 1) != DG_OK) return 0;
    return head_weights_bytes(C, D);
}

// images B.. of a tensor that continues in a second allocation: (second base - first base) in elements, minus the B images in front
template <typename T>
static long long pair_delta(const T* first, const T* second, int32_t B, long long stride) {
    if (!second) return 0;
    return (long long)((reinterpret_cast<intptr_t>(second) - reinterpret_cast<intptr_t>(first)) / (intptr_t)sizeof(T)) - (long long)B * stride;
}

// B images per pass.  feat_pos non-null: a second pass, the call covers nB = 2 B images, the first B from feat / into code / feats_out, the
// rest from / into the *_pos tensors; null: one pass, nB = B
extern "C" int dg_head_forward(int32_t B, int32_t C, int32_t D, int32_t P, const float* feat, const float* feat_pos,
                               const float* w1, const float* b1, const float* w2a, const float* b2a, const float* w2b, const float* b2b,
                               const float* keep1, const float* keep2, const float* keep3, float keep_scale,
                               float* code, float* code_pos, float* feats_out, float* feats_out_pos, void* hidden, void* wscratch,
                               dg_stream_t stream_) {
    const bool two = feat_pos != nullptr;
    if (two && (B < 1 || B > (1 << 20))) return fail(DG_ERR_INVALID, "bad head dimensions");
    const int32_t nB = two ? 2 * B : B;
    if (int rc = head_check(nB, C, D, P)) return rc;
    if (!two && (code_pos || feats_out_pos)) return fail(DG_ERR_INVALID, "code_pos / feats_out_pos without feat_pos (the second pass exists exactly when feat_pos is given)");
    if (!feat || !w1 || !b1 || !code || !wscratch) return fail(DG_ERR_INVALID, "null pointer");
    if (two && (!code_pos || ((feats_out != nullptr) != (feats_out_pos != nullptr)))) return fail(DG_ERR_INVALID, "null pointer of the second pass");
    const bool nonlinear = w2a != nullptr;
    if (nonlinear && (!b2a || !w2b || !b2b)) return fail(DG_ERR_INVALID, "cluster2 needs all four of its tensors");
    hipStream_t s = static_cast<hipStream_t>(stream_);
    DG_HIP(dg_launch_head_prep(w1, w2a, w2b, wscratch, C, D, s));
    DgHeadFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.feat = feat; a.w1 = w1; a.b1 = b1; a.w2a = w2a; a.b2a = b2a; a.w2b = w2b; a.b2b = b2b;
    { const DgHeadWeightLayout L(C, D); const __bf16* w = static_cast<const __bf16*>(wscratch); a.w1_bf = w + L.w1; a.w2a_bf = w + L.w2a; a.w2b_bf = w + L.w2b; }
    a.keep1 = keep1; a.keep2 = keep2; a.keep3 = keep3; a.scale = keep_scale;
    a.code = code; a.feats_out = feats_out; a.hidden = static_cast<__bf16*>(hidden);
    a.B = nB; a.C = C; a.D = D; a.P = P;
    a.Bs = B;
    a.d_feat = pair_delta(feat, feat_pos, B, (long long)C * P);
    a.d_code = pair_delta(code, code_pos, B, (long long)D * P);
    a.d_fo = pair_delta(feats_out, feats_out_pos, B, (long long)C * P);
    DG_HIP(dg_launch_head_fwd(a, s));
    return DG_OK;
}

extern "C" size_t dg_head_workspace_bytes(int32_t B, int32_t C, int32_t D, int32_t P) {
    if (head_check(B, C, D, P) != DG_OK) return 0;
    return dg_head_plan(B, C, D, P).total;
}

extern "C" int dg_head_plan_describe(int32_t B, int32_t C, int32_t D, int32_t P, int32_t* out) {
    if (int rc = head_check(B, C, D, P)) return rc;
    if (!out) return fail(DG_ERR_INVALID, "null pointer");
    const DgHeadPlan h = dg_head_plan(B, C, D, P);
    out[0] = h.dh_route; out[1] = h.dh_blocks; out[2] = h.tiles;
    out[3] = h.wgrad_pair; out[4] = h.wgrad_single;
    out[5] = h.s2a; out[6] = h.s1; out[7] = h.s2b;
    out[8] = h.step_major ? 1 : 0;
    return DG_OK;
}

// feat_pos non-null: the two passes of dg_head_forward, nB = 2 B images (grad_code_pos as code_pos there); null: one pass, nB = B
extern "C" int dg_head_backward(int32_t B, int32_t C, int32_t D, int32_t P, const float* feat, const float* feat_pos, const float* keep1,
                                const float* keep2, float keep_scale, const void* hidden, const void* wscratch, const float* grad_code,
                                const float* grad_code_pos, float* grad_w1, float* grad_b1, float* grad_w2a, float* grad_b2a,
                                float* grad_w2b, float* grad_b2b, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    const bool two = feat_pos != nullptr;
    if (two && (B < 1 || B > (1 << 20))) return fail(DG_ERR_INVALID, "bad head dimensions");
    const int32_t nB = two ? 2 * B : B;
    if (int rc = head_check(nB, C, D, P)) return rc;
    if (!two && grad_code_pos) return fail(DG_ERR_INVALID, "grad_code_pos without feat_pos (the second pass exists exactly when feat_pos is given)");
    if (!feat || !grad_code || !grad_w1 || !grad_b1 || !workspace) return fail(DG_ERR_INVALID, "null pointer");
    if (two && !grad_code_pos) return fail(DG_ERR_INVALID, "null pointer of the second pass");
    const long long d_feat = pair_delta(feat, feat_pos, B, (long long)C * P), d_g = pair_delta(grad_code, grad_code_pos, B, (long long)D * P);
    const bool nonlinear = grad_w2a != nullptr;
    if (nonlinear && (!hidden || !wscratch || !grad_b2a || !grad_w2b || !grad_b2b)) return fail(DG_ERR_INVALID, "null cluster2 pointer");
    const DgHeadPlan h = dg_head_plan(nB, C, D, P);       // (the kernels' own: sizes, splits and the route of every launch below)
    if (workspace_bytes < h.total) return fail(DG_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, h.total);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    DgHeadReduceArgs red;
    memset(&red, 0, sizeof(red));
    auto reduce = [&](const float* part, float* out, float* out2, int n, int splits, float scale) {
        red.jobs[red.njobs++] = DgHeadReduceJob{part, out, out2, n, splits, scale};
    };
    // d W1[d][k] = scale * keep1[b][k] * sum_p g[d][p] f[k][p]      (with cluster2: in the launch of d W2a below, which reads the same f)
    if (!nonlinear) {
        DgHeadWgradArgs w{grad_code, feat, keep1, F32(h.p1), nB, D, C, P, h.s1};
        w.A2 = nullptr; w.keep_2 = nullptr; w.part2 = nullptr; w.M2 = 0;
        w.Bs = B; w.dA = d_g; w.dB = d_feat; w.dA2 = 0;
        DG_HIP(dg_launch_head_wgrad(w, h.wgrad_single, false, false, s));
        reduce(F32(h.p1), grad_w1, nullptr, D * C, h.s1, keep1 ? keep_scale : 1.f);
    }
    if (!nonlinear) {        // d b1 = row sums of d code
        DG_HIP(dg_launch_head_rowsum(grad_code, false, grad_b1, nullptr, nB, D, P, s, B, d_g));
        DG_HIP(dg_launch_head_reduce(red, s));
        return DG_OK;
    }
    __bf16* dh = reinterpret_cast<__bf16*>(ws + h.dh);
    const __bf16* w2bT = static_cast<const __bf16*>(wscratch) + DgHeadWeightLayout(C, D).w2bT;
    DgHeadDhArgs d{grad_code, w2bT, static_cast<const __bf16*>(hidden), dh, F32(h.pbd), F32(h.pb2a), nB, C, D, P, B, d_g};
    d.gcode_bf = h.wgrad_pair == DG_HEAD_WGRAD_ONE_PASS ? reinterpret_cast<__bf16*>(ws + h.gbf) : nullptr;
    d.step_major = h.step_major ? 1 : 0;
    // d W2b = d code x hidden^T needs nothing of k_head_dh: it runs BESIDE it on the library's second stream where there is one (fork
    // / join by events, capturable): two launches that each leave most of the chip idle (27 and 37 us at the paired headline shape)
    DgHeadWgradArgs wb{grad_code, hidden, nullptr, F32(h.p2b), nB, D, C, P, h.s2b};
    wb.A2 = nullptr; wb.keep_2 = nullptr; wb.part2 = nullptr; wb.M2 = 0;
    wb.Bs = B; wb.dA = d_g; wb.dB = 0; wb.dA2 = 0;
    const bool w2b_fused = h.dh_route == DG_HEAD_DH_FUSED;     // (k_head_dh2: the product rides in the d hidden launch - no second launch, no second stream)
    if (w2b_fused) d.part_w2b = F32(h.p2b);
    std::optional<SideRegion> side_o;
    if (!w2b_fused) side_o.emplace(s);
    const bool side = side_o && *side_o;
    if (side) {
        DG_HIP(side_o->fork());
        DG_HIP(dg_launch_head_wgrad(wb, h.wgrad_single, false, true, side_o->stream()));
        DG_HIP(side_o->record_join());
    }
    DG_HIP(dg_launch_head_dh(d, h, s));
    reduce(F32(h.pbd), grad_b1, grad_b2b, D, nB * h.tiles, 1.f);       // d b1 = d b2b = row sums of d code
    reduce(F32(h.pb2a), grad_b2a, nullptr, C, nB * h.tiles, 1.f);
    if (!side && !w2b_fused) DG_HIP(dg_launch_head_wgrad(wb, h.wgrad_single, false, true, s));
    reduce(F32(h.p2b), grad_w2b, nullptr, D * C, h.s2b, 1.f);
    DgHeadWgradArgs wa{dh, feat, keep2, F32(h.p2a), nB, C, C, P, h.s2a, grad_code, keep1, F32(h.p1), D};
    wa.Bs = B; wa.dA = 0; wa.dB = d_feat; wa.dA2 = d_g;
    wa.A2h = d.gcode_bf;
    wa.a_step_major = d.step_major;
    DG_HIP(dg_launch_head_wgrad(wa, h.wgrad_pair, true, false, s));
    reduce(F32(h.p2a), grad_w2a, nullptr, C * C, h.s2a, keep2 ? keep_scale : 1.f);
    reduce(F32(h.p1), grad_w1, nullptr, D * C, h.s2a, keep1 ? keep_scale : 1.f);
    if (side) DG_HIP(side_o->join());
    DG_HIP(dg_launch_head_reduce(red, s));         // all five reductions in one launch
    return DG_OK;
}

// ---- d image_feat (opt-in): behind dg_head_backward* on the same workspace and stream
extern "C" size_t dg_head_input_workspace_bytes(int32_t C, int32_t D) {
    if (head_check(1, C, D, 1) != DG_OK) return 0;
    return DgHeadDxLayout(C, D, true).elems * 2;
}

// d image_feat, plus - where grad_feats_out of a pass is given - what reached the returned feats: grad_feat += keep_scale keep3 grad_feats_out,
// in the launch's epilogue.  grad_code_pos non-null: the two passes of dg_head_backward, nB = 2 B images; null: one pass, nB = B
extern "C" int dg_head_backward_input(int32_t B, int32_t C, int32_t D, int32_t P, const float* w1, const float* w2a, const float* keep1,
                                      const float* keep2, const float* keep3, float keep_scale, const void* hidden,
                                      const float* grad_code, const float* grad_code_pos, const float* grad_feats_out,
                                      const float* grad_feats_out_pos, const void* workspace, size_t workspace_bytes, float* grad_feat,
                                      float* grad_feat_pos, void* input_workspace, size_t input_workspace_bytes, dg_stream_t stream_) {
    const bool two = grad_code_pos != nullptr;
    if (two && (B < 1 || B > (1 << 20))) return fail(DG_ERR_INVALID, "bad head dimensions");
    const int32_t nB = two ? 2 * B : B;
    if (int rc = head_check(nB, C, D, P)) return rc;
    if (!two && (grad_feats_out_pos || grad_feat_pos))
        return fail(DG_ERR_INVALID, "grad_feats_out_pos / grad_feat_pos without grad_code_pos (the second pass exists exactly when grad_code_pos is given)");
    if ((((uintptr_t)grad_feats_out | (uintptr_t)grad_feats_out_pos) & 15) || ((uintptr_t)keep3 & 3))
        return fail(DG_ERR_INVALID, "grad_feats_out must be 16-byte aligned, keep3 4-byte aligned");
    if ((grad_feats_out && !grad_feat) || (grad_feats_out_pos && !grad_feat_pos))
        return fail(DG_ERR_INVALID, "grad_feats_out of a pass whose grad_feat is null");
    if (!w1 || !grad_code || !input_workspace) return fail(DG_ERR_INVALID, "null pointer");
    if (!grad_feat && !grad_feat_pos) return fail(DG_ERR_INVALID, "null pointer (grad_code of both passes, grad_feat of one at least)");
    const bool nonlinear = w2a != nullptr;
    if (nonlinear && (!hidden || !workspace)) return fail(DG_ERR_INVALID, "cluster2's half needs `hidden` and the workspace dg_head_backward left d hidden in");
    const DgHeadPlan h = dg_head_plan(nB, C, D, P);       // (the plan dg_head_backward followed: where d hidden is and how it is laid out)
    if (nonlinear && workspace_bytes < h.total) return fail(DG_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, h.total);
    const DgHeadDxLayout L(C, D, nonlinear);
    if (input_workspace_bytes < L.elems * 2) return fail(DG_ERR_WORKSPACE, "input workspace %zu < required %zu bytes", input_workspace_bytes, L.elems * 2);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    DG_HIP(dg_launch_head_dx_prep(w1, w2a, input_workspace, C, D, s));
    DgHeadDxArgs a;
    memset(&a, 0, sizeof(a));
    a.gcode = grad_code;
    a.dh = nonlinear ? reinterpret_cast<const __bf16*>(static_cast<const char*>(workspace) + h.dh) : nullptr;
    a.wT = static_cast<const __bf16*>(input_workspace);
    a.keep1 = keep1; a.keep2 = nonlinear ? keep2 : nullptr; a.scale = keep_scale;
    a.dx = grad_feat; a.dx2 = grad_feat_pos;
    a.B = nB; a.C = C; a.D = D; a.P = P;
    a.Bs = B; a.d_gcode = pair_delta(grad_code, grad_code_pos, B, (long long)D * P);
    a.b0 = grad_feat ? 0 : B;                             // (a pass without grad_feat: its images are not walked)
    a.nb = (grad_feat && grad_feat_pos) ? nB : B;
    a.step_major = (nonlinear && h.step_major) ? 1 : 0;
    a.gfeats = grad_feats_out; a.gfeats2 = grad_feats_out_pos; a.keep3 = keep3;
    DG_HIP(dg_launch_head_dx(a, s));
    return DG_OK;
}
