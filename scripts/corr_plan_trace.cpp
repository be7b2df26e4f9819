// Recorded-launch trace of the correlation loss's host unit (depthg_amd/csrc/dg_api_corr.hip), without a GPU.
// The unit is compiled for the host and linked against the recording stand-ins below for everything it calls outward: every
// dg_launch_*, side_stream_for, hipEventRecord, hipStreamWaitEvent, hipMemsetAsync, fail and the error string; the dg_*_supported predicates are the
// tree's own (predicates.inc: their text, lifted from dg_corr2.hip and dg_small.hip by the build script).  No call reaches the HIP runtime; the workspace and all tensors are fixed made-up
// addresses, and the unit zeroes its argument blocks before it fills them, so two builds of the unit give records that compare byte
// for byte.  main() walks a grid of descriptors and calls every entry point for each (refused calls included), prints one line per
// descriptor (calls, launches, FNV-1a digest of return codes, error texts, workspace sizes, launch names, streams and argument
// bytes), then the per-route call counts, and exits non-zero if a route the grid has to reach was not reached.  A last pass lets
// every launcher fail in turn, so that the texts and the records of failed launches (the side stream's join among them) are compared too.
// Built and run by scripts/corr_plan_trace.sh.      corr_plan_trace [--desc N]   (--desc N: print descriptor N's records in full)
#include "dg_api.h"
#include "dg_corr_args.h"

#include <cstdarg>
#include <map>
#include <string>
#include <vector>

// ---- records
static hipStream_t const CALLER = reinterpret_cast<hipStream_t>(0x7000), SIDE = reinterpret_cast<hipStream_t>(0x7100);
static uint64_t g_hash = 1469598103934665603ull;
static long g_launches = 0;
static bool g_verbose = false, g_side_on = true;
static const dg_corr_desc* g_desc = nullptr;          // the descriptor of the call in flight (route counting only)
static std::map<std::string, long> g_routes;
static std::string g_last_main;                        // the fused launch of the call in flight
static void route(const std::string& r) { ++g_routes[r]; }
static long g_corr2_declined = 0;                     // dg_launch_corr2 asked for a launch it does not support (not part of the digest)
// failure injection: the launcher of this name returns an error (after its record); the fused launch's two launchers only where they
// are that launch (g_fail_main), and their text then stays out of the digest: it names the expression of the call site, which
// differs between revisions that pass the launch through launch_main in different ways (printed as a note instead)
static std::string g_fail_name;
static bool g_failed = false, g_failed_main = false;
static hipError_t result(const char* name, bool is_main = false) {
    if (g_fail_name != name) return hipSuccess;
    g_failed = true; g_failed_main = is_main;
    return hipErrorInvalidValue;
}
static void mix(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { g_hash ^= b[i]; g_hash *= 1099511628211ull; }
}
static char stream_tag(hipStream_t s) { return s == CALLER ? 'C' : (s == SIDE ? 'S' : '?'); }
static void record(const char* name, hipStream_t s, const void* bytes, size_t n) {
    const char tag = stream_tag(s);
    mix(name, strlen(name) + 1); mix(&tag, 1); mix(&n, sizeof(n)); mix(bytes, n);
    ++g_launches;
    if (g_verbose) {
        printf("    %s %c %zu ", name, tag, n);
        for (size_t i = 0; i < n; ++i) printf("%02x", static_cast<const unsigned char*>(bytes)[i]);
        printf("\n");
    }
}
template <class T> static void record(const char* name, hipStream_t s, const T& a) { record(name, s, &a, sizeof(T)); }
template <class T> static void record(const char* name, hipStream_t s, const T& a, std::initializer_list<long long> extra) {
    std::vector<unsigned char> b(sizeof(T) + extra.size() * sizeof(long long));
    memcpy(b.data(), &a, sizeof(T));
    size_t o = sizeof(T);
    for (long long v : extra) { memcpy(b.data() + o, &v, sizeof(v)); o += sizeof(v); }
    record(name, s, b.data(), b.size());
}
static void record_values(const char* name, hipStream_t s, std::initializer_list<long long> v) { record(name, s, v.begin(), v.size() * sizeof(long long)); }
static long long addr(const void* p) { return (long long)reinterpret_cast<uintptr_t>(p); }

// ---- error reporting (dg_api_aux.hip)
thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* hipGetErrorString(hipError_t e) {
    return e == hipSuccess ? "no error" : (e == hipErrorNotSupported ? "operation not supported" : (e == hipErrorInvalidValue ? "invalid argument" : "other error"));
}

// ---- the side stream and its events
static SideStream g_side;
SideStream* side_stream_for(hipStream_t caller) {
    record_values("side_stream_for", caller, {g_side_on ? 1 : 0});
    if (!g_side_on) return nullptr;
    g_side.s = SIDE;
    g_side.fork = reinterpret_cast<hipEvent_t>(0x8000); g_side.join = reinterpret_cast<hipEvent_t>(0x8100);
    g_side.mid[0] = reinterpret_cast<hipEvent_t>(0x8200); g_side.mid[1] = reinterpret_cast<hipEvent_t>(0x8300);
    return &g_side;
}
extern "C" hipError_t hipEventRecord(hipEvent_t ev, hipStream_t s) { record_values("hipEventRecord", s, {addr(ev)}); return result("hipEventRecord"); }
extern "C" hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t ev, unsigned int flags) {
    record_values("hipStreamWaitEvent", s, {addr(ev), (long long)flags});
    return result("hipStreamWaitEvent");
}

// ---- the predicates of the tree under test
#include "predicates.inc"

// ---- the launchers
static void widths(int KF, int KD) { route("KF" + std::to_string(KF)); route("KD" + std::to_string(KD)); }
hipError_t dg_launch_corr(const DgCorrArgs& a, int KF, int KD, int nwaves, int mode, hipStream_t s) {
    record("dg_launch_corr", s, a, {KF, KD, nwaves, mode});
    widths(KF, KD);
    if (mode != 2) {
        g_last_main = "k_corr_main";
        route(nwaves == 8 ? "rf8" : "rf4");
        if (mode == 1) route("grad_k_corr_main");
        if (a.njobs > 0 && a.jobs[a.njobs - 1].kind == DG_JOB_DEPTH) route("depth_as_job");
        if (g_desc && (g_desc->flags & DG_IDENTITY_GRID) && mode == 1 && !a.jobs[0].maskbits) route("dense_sign_masks");
    } else {
        route(a.jobs[0].kind == DG_JOB_DEPTH ? "materialize_depth" : "materialize_pairset");
    }
    return result("dg_launch_corr", mode != 2);
}
hipError_t dg_launch_corr2(const DgCorrArgs& a, int KF, int KD, hipStream_t s) {
    if (!dg_corr2_supported(a, KF, KD)) { ++g_corr2_declined; return hipErrorNotSupported; }
    record("dg_launch_corr2", s, a, {KF, KD});
    widths(KF, KD);
    g_last_main = "k_corr2";
    route("grad_k_corr2");
    if (a.jobs[0].fold) route("fold");
    else if (g_desc && (g_desc->flags & DG_POINTWISE)) route("pointwise_k_corr2_unfolded");
    if (a.half_tiles) route("half");
    if (g_desc && (g_desc->flags & DG_IDENTITY_GRID) && !a.jobs[0].maskbits) route("dense_sign_masks");
    if (a.gr_list) {
        route("grouped");
        if (a.B == 8) route("grouped_B8");
        if (a.B == 64) route("grouped_B64");
        if (g_desc && g_desc->h == 28 && g_desc->w == 28 && (g_desc->flags & DG_SHARED_COORDS)) route("grouped_28x28_shared");
        if (g_desc && g_desc->n_neg == 1) route("grouped_N1");
        if (g_desc && g_desc->n_neg > 1) route("grouped_N2plus");
    }
    return result("dg_launch_corr2", true);
}
hipError_t dg_launch_gs(const DgGsArgs& a, const uint32_t* dep_maskbits, hipStream_t s, bool depth_only, bool half_out) {
    record("dg_launch_gs", s, a, {addr(dep_maskbits), depth_only ? 1 : 0, half_out ? 1 : 0});
    if (a.dep_blocks > 0 && !depth_only) route("depth_as_gs_blocks");
    if (depth_only) route(s == SIDE ? "masked_depth_side_stream" : "masked_depth_caller_stream");
    return result("dg_launch_gs");
}
hipError_t dg_launch_finish(const DgFinishArgs& a, hipStream_t s) { record("dg_launch_finish", s, a); return result("dg_launch_finish"); }
hipError_t dg_launch_transpose(const DgTransposeArgs& a, int B, hipStream_t s) {
    record("dg_launch_transpose", s, a, {B});
    if (a.nmaps == 5) route("xop");          // (the plan's xop >= 0: the intra feature map is the fifth map, or src_x below)
    return result("dg_launch_transpose");
}
hipError_t dg_launch_gather(const DgGatherArgs& a, int maxK, hipStream_t s) {
    record("dg_launch_gather", s, a, {maxK});
    route("general_blobs");
    if (g_desc && (g_desc->flags & DG_LINE_GRID)) route("general_line_grid");
    else if (g_desc && g_desc->S >= 14) route("general_S14plus");
    route(a.direct ? "general_plane_sampler" : "general_channel_last");
    if (a.cd.T > 0) route("exact_masks_small_sample_grid");
    return result("dg_launch_gather");
}
hipError_t dg_launch_cd_mask(const DgCdMaskArgs& a, hipStream_t s) { record("dg_launch_cd_mask", s, a); route("dense_exact_raw"); return result("dg_launch_cd_mask"); }
hipError_t dg_launch_cd_mask3(const DgCdMask3Args& a, hipStream_t s) {
    record("dg_launch_cd_mask3", s, a);
    route("dense_exact_split");
    route(s == SIDE ? "mask3_side_stream" : (g_side_on ? "mask3_caller_stream_with_side" : "mask3_caller_stream_no_side"));
    return result("dg_launch_cd_mask3");
}
hipError_t dg_launch_plane_sample(const DgPlaneArgs& a, hipStream_t s) {
    record("dg_launch_plane_sample", s, a);
    if (a.feats_bf16) route("small_plane_sampler");
    if (a.src_x) route("xop");
    return result("dg_launch_plane_sample");
}
hipError_t dg_launch_colmean(const DgColmeanArgs& a, hipStream_t s) { record("dg_launch_colmean", s, a); return result("dg_launch_colmean"); }
hipError_t dg_launch_prep_dense(const DgDenseArgs& a, hipStream_t s) {
    record("dg_launch_prep_dense", s, a);
    route(a.code_split ? "dense_pointwise" : "dense_plain");
    if (a.fkeep[0] || a.fkeep[1]) route("feat_keep");
    return result("dg_launch_prep_dense");
}
hipError_t dg_launch_rowmean(const DgRowmeanArgs& a, hipStream_t s) { record("dg_launch_rowmean", s, a); return result("dg_launch_rowmean"); }
hipError_t dg_launch_set_stash(char* blobs, int B, int ntiles, size_t blob_bytes, int off, const float* rvec, int P, int Ppad, hipStream_t s) {
    record_values("dg_launch_set_stash", s, {addr(blobs), B, ntiles, (long long)blob_bytes, off, addr(rvec), P, Ppad});
    route("materialize_after_fold");
    return result("dg_launch_set_stash");
}
hipError_t dg_launch_scatter(const DgScatterArgs& a, hipStream_t s) {
    record("dg_launch_scatter", s, a);
    route(a.naxpy > 0 ? "backward_small_merged" : (a.dense ? "backward_dense" : "backward_general"));
    return result("dg_launch_scatter");
}
hipError_t dg_launch_pre_general(const DgPreArgs& a, hipStream_t s) {
    record("dg_launch_pre_general", s, a);
    if (a.count > 0) route(a.state ? "draw_with_state" : "draw_without_state");
    return result("dg_launch_pre_general");
}
hipError_t dg_launch_corr_small(const DgSmallArgs& a, hipStream_t s) {
    record("dg_launch_corr_small", s, a);
    g_last_main = "k_corr_small";
    route(a.nsplit == 2 ? "small_nsplit2" : "small_nsplit1");
    if (a.mat) route(a.mat_t < 0 ? "materialize_depth" : "materialize_pairset");
    return result("dg_launch_corr_small");
}
hipError_t dg_launch_small_finish(const DgSmallArgs& a, hipStream_t s) { record("dg_launch_small_finish", s, a); return result("dg_launch_small_finish"); }
hipError_t dg_launch_gather_rows(const DgGatherRowsArgs& a, hipStream_t s) {
    record("dg_launch_gather_rows", s, a);
    if (g_desc && g_desc->code_h) route("small_gather_code_maps_of_another_size");
    if (g_desc && g_desc->h * g_desc->w > 1024) route("small_gather_maps_above_1024_pixels");
    return result("dg_launch_gather_rows");
}
hipError_t dg_launch_sampled_sumsq(const float* feats, const float* coords, const int64_t* srcidx, float* out, int B, int C, int h, int w, int S, int Sh,
                                   int accumulate, hipStream_t s) {
    record_values("dg_launch_sampled_sumsq", s, {addr(feats), addr(coords), addr(srcidx), addr(out), B, C, h, w, S, Sh, accumulate});
    return result("dg_launch_sampled_sumsq");
}
extern "C" hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) {
    record_values("hipMemsetAsync", s, {addr(dst), value, (long long)bytes});
    return result("hipMemsetAsync");
}
hipError_t dg_launch_cd_hist(const DgCdHistArgs& a, bool rows, hipStream_t s) { record("dg_launch_cd_hist", s, a, {rows ? 1 : 0}); return result("dg_launch_cd_hist"); }
hipError_t dg_launch_normalize_split(const float* src, int B, int C, int P, int nchunks, int chunk_c, float* const* dst, hipStream_t s) {
    std::vector<long long> v = {addr(src), B, C, P, nchunks, chunk_c};
    for (int k = 0; k < nchunks; ++k) v.push_back(addr(dst[k]));
    record("dg_launch_normalize_split", s, v.data(), v.size() * sizeof(long long));
    return result("dg_launch_normalize_split");
}

// ---- the entry points under test
extern "C" int dg_prof_main_span(void* span);
extern "C" int dg_corr_intra_folded(const dg_corr_desc* desc);
extern "C" const char* dg_corr_main_kernel_name(const dg_corr_desc* desc);
extern "C" int dg_corr_relaunch_main(const dg_corr_desc* desc, const int64_t* perms, void* workspace, size_t workspace_bytes, dg_stream_t stream_);

// ---- the driver
template <class T> static T* fake(uintptr_t a) { return reinterpret_cast<T*>(a); }
static char* const WS = fake<char>(0x100000000000ull);
static float* const FEATS = fake<float>(0x200000000000ull);
static float* const FEATS_POS = fake<float>(0x210000000000ull);
static float* const CODE = fake<float>(0x220000000000ull);
static float* const CODE_POS = fake<float>(0x230000000000ull);
static float* const DEPTH = fake<float>(0x240000000000ull);
static float* const COORDS1 = fake<float>(0x250000000000ull);
static float* const COORDS2 = fake<float>(0x260000000000ull);
static int64_t* const PERMS = fake<int64_t>(0x270000000000ull);
static float* const OUT = fake<float>(0x280000000000ull);
static float* const GRAD = fake<float>(0x290000000000ull);
static float* const GCODE = fake<float>(0x2a0000000000ull);
static float* const GCODE_POS = fake<float>(0x2b0000000000ull);
static float* const OUT_CD = fake<float>(0x2c0000000000ull);
static float* const OUT_LOSS = fake<float>(0x2d0000000000ull);
static float* const KEEP = fake<float>(0x2e0000000000ull);
static float* const KEEP_POS = fake<float>(0x2f0000000000ull);
static float* const FEAT_INV = fake<float>(0x300000000000ull);
static void* const STATE = fake<void>(0x310000000000ull);
static float* const INTRA = fake<float>(0x360000000000ull);
static int64_t* const HIST = fake<int64_t>(0x370000000000ull);

static long g_calls = 0, g_desc_calls = 0;
static void begin(const dg_corr_desc* d, const char* entry) {
    g_desc = d; g_err[0] = 0; g_last_main.clear();
    ++g_calls; ++g_desc_calls;
    route(std::string("entry_") + entry);
    mix(entry, strlen(entry) + 1);
    if (g_verbose) printf("  %s\n", entry);
}
static std::map<std::string, long> g_main_texts;      // texts of a failed fused launch (notes, not part of the digest)
static int end(int rc) {
    mix(&rc, sizeof(rc));
    if (g_failed_main) ++g_main_texts[g_err];
    else mix(g_err, strlen(g_err) + 1);
    if (g_failed) route("launch_failed");
    g_failed = g_failed_main = false;
    if (rc != DG_OK) route("refused");
    if (g_verbose) printf("    -> %d %s\n", rc, g_err);
    return rc;
}
#define CALL(entry, ...) (begin(d, #entry), end(entry(__VA_ARGS__)))

static int g_mismatch = 0;
static void run_desc(const dg_corr_desc* d, bool refusals) {
    hipStream_t st = CALLER;
    begin(d, "dg_corr_workspace_bytes");
    const size_t ws = dg_corr_workspace_bytes(d);
    mix(&ws, sizeof(ws));
    if (g_verbose) printf("    -> %zu bytes\n", ws);
    const int T = d ? 2 + d->n_neg : 2;
    for (int side = 1; side >= 0; --side) {
        g_side_on = side != 0;
        if (CALL(dg_corr_forward, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, OUT, WS, ws, st) == DG_OK) {
            route(d->n_neg == 0 ? "n_neg_0" : (d->n_neg == 1 ? "n_neg_1" : (d->n_neg == DG_MAX_NEG ? "n_neg_max" : "n_neg_other")));
            if (d->flags & DG_STABALIZE) route("stabalize");
            if (!(d->flags & DG_ZERO_CLAMP)) route("no_zero_clamp");
        }
        if (CALL(dg_corr_forward_extnorm, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, FEAT_INV, OUT, WS, ws, st) == DG_OK) route("feat_inv");
        CALL(dg_corr_forward_draw, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, 1234u, STATE, OUT, WS, ws, st);
        CALL(dg_corr_forward_draw, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, 99u, nullptr, OUT, WS, ws, st);
        CALL(dg_corr_forward_masked, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, 0, 0u, nullptr, nullptr, nullptr, 1.f, OUT, WS, ws, st);
        CALL(dg_corr_forward_masked, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, 1, 7u, STATE, KEEP, KEEP_POS, 1.25f, OUT, WS, ws, st);
        CALL(dg_corr_forward_masked, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, 1, 7u, nullptr, nullptr, KEEP_POS, 2.f, OUT, WS, ws, st);
    }
    g_side_on = true;
    // the intra-feature entry on its own, larger workspace: one accepted call (where the descriptor is served), one without the map
    begin(d, "dg_corr_workspace_bytes_intra_feats");
    const size_t wsx = dg_corr_workspace_bytes_intra_feats(d);
    mix(&wsx, sizeof(wsx));
    if (g_verbose) printf("    -> %zu bytes\n", wsx);
    CALL(dg_corr_forward_intra_feats, d, FEATS, FEATS_POS, CODE, CODE_POS, nullptr, COORDS1, COORDS2, PERMS, 1, 5u, nullptr, INTRA, OUT, WS, wsx, st);
    CALL(dg_corr_forward_intra_feats, d, FEATS, FEATS_POS, CODE, CODE_POS, nullptr, COORDS1, COORDS2, PERMS, 0, 0u, nullptr, nullptr, OUT, WS, wsx, st);
    CALL(dg_corr_backward, d, GRAD, COORDS1, COORDS2, PERMS, GCODE, GCODE_POS, WS, ws, st);
    CALL(dg_corr_backward_total, d, GRAD, COORDS1, COORDS2, PERMS, GCODE, GCODE_POS, WS, ws, st);
    for (int which = -1; which < T; ++which) {
        CALL(dg_corr_materialize, d, which, OUT_CD, OUT_LOSS, WS, ws, st);
        CALL(dg_corr_materialize_shared, d, which, PERMS, OUT_CD, nullptr, WS, ws, st);
    }
    CALL(dg_corr_materialize_shared, d, 0, PERMS, nullptr, OUT_LOSS, WS, ws, st);
    CALL(dg_corr_materialize, d, 0, nullptr, nullptr, WS, ws, st);
    CALL(dg_corr_cd_hist, d, 0, T, PERMS, 64, -1.f, 1.f, HIST, WS, ws, st);
    const int rc_relaunch = CALL(dg_corr_relaunch_main, d, PERMS, WS, ws, st);
    const std::string relaunched = g_last_main;
    begin(d, "dg_corr_intra_folded");
    end(dg_corr_intra_folded(d));
    begin(d, "dg_corr_main_kernel_name");
    const char* name = dg_corr_main_kernel_name(d);
    mix(name ? name : "(null)", strlen(name ? name : "(null)") + 1);
    if (g_verbose) printf("    -> %s\n", name ? name : "(null)");
    if (rc_relaunch == DG_OK && (!name || relaunched != name)) {
        ++g_mismatch;
        fprintf(stderr, "dg_corr_main_kernel_name says %s, dg_corr_relaunch_main launched %s\n", name ? name : "(null)", relaunched.c_str());
    }
    if (!refusals) return;
    // calls that must be refused: every null pointer, a short workspace, arguments out of range
    const size_t shrt = ws ? ws - 1 : 0;
    const float* in[7] = {FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2};
    for (int k = 0; k < 7; ++k) {
        const float* a[7];
        for (int i = 0; i < 7; ++i) a[i] = i == k ? nullptr : in[i];
        CALL(dg_corr_forward, d, a[0], a[1], a[2], a[3], a[4], a[5], a[6], PERMS, OUT, WS, ws, st);
    }
    CALL(dg_corr_forward, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, nullptr, OUT, WS, ws, st);
    CALL(dg_corr_forward, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, nullptr, WS, ws, st);
    CALL(dg_corr_forward, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, OUT, nullptr, ws, st);
    CALL(dg_corr_forward, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, OUT, WS, shrt, st);
    CALL(dg_corr_forward_extnorm, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, nullptr, OUT, WS, ws, st);
    CALL(dg_corr_forward_draw, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, nullptr, 1u, STATE, OUT, WS, ws, st);
    CALL(dg_corr_forward_masked, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, nullptr, 1, 1u, STATE, nullptr, nullptr, 1.f, OUT, WS, ws, st);
    CALL(dg_corr_forward_masked, d, FEATS, FEATS_POS, CODE, CODE_POS, DEPTH, COORDS1, COORDS2, PERMS, 1, 1u, STATE, KEEP, nullptr, 0.f, OUT, WS, ws, st);
    CALL(dg_corr_backward, d, nullptr, COORDS1, COORDS2, PERMS, GCODE, GCODE_POS, WS, ws, st);
    CALL(dg_corr_backward_total, d, nullptr, COORDS1, COORDS2, PERMS, GCODE, GCODE_POS, WS, ws, st);
    CALL(dg_corr_backward, d, GRAD, nullptr, COORDS2, PERMS, GCODE, GCODE_POS, WS, ws, st);
    CALL(dg_corr_backward, d, GRAD, COORDS1, nullptr, PERMS, GCODE, GCODE_POS, WS, ws, st);
    CALL(dg_corr_backward, d, GRAD, COORDS1, COORDS2, nullptr, GCODE, GCODE_POS, WS, ws, st);
    CALL(dg_corr_backward, d, GRAD, COORDS1, COORDS2, PERMS, nullptr, GCODE_POS, WS, ws, st);
    CALL(dg_corr_backward, d, GRAD, COORDS1, COORDS2, PERMS, GCODE, nullptr, WS, ws, st);
    CALL(dg_corr_backward, d, GRAD, COORDS1, COORDS2, PERMS, GCODE, GCODE_POS, nullptr, ws, st);
    CALL(dg_corr_backward_total, d, GRAD, COORDS1, COORDS2, PERMS, GCODE, GCODE_POS, WS, shrt, st);
    CALL(dg_corr_materialize, d, -2, OUT_CD, OUT_LOSS, WS, ws, st);
    CALL(dg_corr_materialize, d, T, OUT_CD, OUT_LOSS, WS, ws, st);
    CALL(dg_corr_materialize, d, 0, OUT_CD, OUT_LOSS, nullptr, ws, st);
    CALL(dg_corr_materialize_shared, d, 1, PERMS, OUT_CD, OUT_LOSS, WS, shrt, st);
    CALL(dg_corr_relaunch_main, d, nullptr, WS, ws, st);
    CALL(dg_corr_relaunch_main, d, PERMS, nullptr, ws, st);
    CALL(dg_corr_relaunch_main, d, PERMS, WS, shrt, st);
}

static int g_index = 0, g_only = -1;
static void visit(const dg_corr_desc* d, bool refusals, const char* note = "") {
    const int idx = g_index++;
    if (g_only >= 0 && idx != g_only) return;
    g_verbose = g_only >= 0;
    const uint64_t h0 = g_hash;
    const long l0 = g_launches;
    g_desc_calls = 0;
    g_hash = 1469598103934665603ull;
    if (d) printf("desc %d B=%d C=%d D=%d h=%d w=%d S=%d N=%d flags=0x%03x code=%dx%d %s\n", idx, d->B, d->C, d->D, d->h, d->w, d->S, d->n_neg, d->flags,
                  d->code_h, d->code_w, note);
    else printf("desc %d null\n", idx);
    run_desc(d, refusals);
    printf("desc %d calls=%ld launches=%ld digest=%016llx\n", idx, g_desc_calls, g_launches - l0, (unsigned long long)g_hash);
    const uint64_t h = g_hash;
    g_hash = h0;
    mix(&h, sizeof(h));
}

static dg_corr_desc make_desc(int B, int C, int D, int h, int w, int S, int N, uint32_t flags, int ch = 0, int cw = 0) {
    dg_corr_desc d;
    memset(&d, 0, sizeof(d));
    d.B = B; d.C = C; d.D = D; d.h = h; d.w = w; d.S = S; d.n_neg = N; d.flags = flags;
    d.depth_h = 224; d.depth_w = 208;
    d.shift_intra = 0.18f; d.shift_inter = 0.46f; d.shift_neg = 0.12f; d.shift_depth = 0.05f;
    d.w_intra = 0.58f; d.w_inter = 0.63f; d.w_neg = 0.67f; d.w_depth = 0.04f;
    d.code_h = ch; d.code_w = cw;
    return d;
}

struct Shape { int C, D, h, w, S; uint32_t grid; int ch, cw; int Bs[3]; };
static const uint32_t DENSE = DG_SHARED_COORDS | DG_IDENTITY_GRID;
static const Shape kShapes[] = {
    // the fused small grid: S = 11 (one block per image and pair-set) and S = 12 (two), both samplers, every width
    {384, 70, 28, 28, 11, 0, 0, 0, {3, 8, 0}},
    {384, 70, 28, 28, 12, 0, 0, 0, {3, 16, 0}},
    {2048, 128, 28, 28, 12, 0, 0, 0, {2, 0, 0}},
    {100, 90, 28, 28, 11, DG_SHARED_COORDS, 0, 0, {4, 0, 0}},
    {384, 70, 40, 40, 12, 0, 0, 0, {2, 0, 0}},                  // maps above 1024 pixels: channel-last copies + gather
    {384, 70, 28, 28, 11, 0, 14, 14, {2, 0, 0}},                // code maps of another size: the same
    {768, 96, 20, 24, 5, 0, 0, 0, {5, 0, 0}},
    {384, 70, 28, 28, 40, DG_LINE_GRID, 0, 0, {2, 0, 0}},
    // general coordinates into blobs: S = 14 and above, the line grid, 4 and 8 waves per block, every width
    {384, 70, 28, 28, 14, 0, 0, 0, {3, 16, 0}},
    {384, 70, 28, 28, 14, DG_SHARED_COORDS, 0, 0, {8, 0, 0}},
    {768, 70, 28, 28, 14, 0, 0, 0, {2, 0, 0}},
    {384, 128, 28, 28, 16, 0, 0, 0, {2, 0, 0}},
    {100, 64, 28, 28, 16, 0, 0, 0, {2, 0, 0}},
    {384, 70, 40, 40, 20, 0, 0, 0, {2, 65, 0}},
    {384, 70, 28, 28, 200, DG_LINE_GRID, 0, 0, {2, 0, 0}},
    {384, 70, 32, 32, 24, 0, 16, 16, {2, 0, 0}},
    {384, 70, 80, 80, 14, 0, 0, 0, {1, 0, 0}},                  // code maps above 4096 pixels: the backward is refused
    {384, 70, 28, 28, 17, DG_SHARED_COORDS, 0, 0, {8, 64, 0}},  // ragged row block of two tiles: grouped
    // the dense identity grid
    {384, 70, 28, 28, 28, DENSE, 0, 0, {8, 64, 3}},
    {384, 70, 14, 14, 14, DENSE, 0, 0, {16, 0, 0}},
    {384, 70, 40, 40, 40, DENSE, 0, 0, {8, 0, 0}},
    {768, 70, 28, 28, 28, DENSE, 0, 0, {8, 0, 0}},
    {384, 128, 16, 16, 16, DENSE, 0, 0, {4, 0, 0}},
    {100, 64, 12, 12, 12, DENSE, 0, 0, {4, 0, 0}},
    {384, 96, 28, 28, 28, DENSE, 0, 0, {8, 0, 0}},
    {384, 70, 64, 64, 64, DENSE, 0, 0, {2, 72, 0}},
};

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "--desc")) g_only = atoi(argv[2]);
    // descriptors make_plan refuses, one per message
    {
        visit(nullptr, true);
        const dg_corr_desc bad[] = {
            make_desc(0, 384, 70, 28, 28, 11, 1, 0), make_desc(2, 384, 70, 28, 28, 0, 1, 0), make_desc(2, 384, 70, 28, 28, 11, -1, 0),
            make_desc(2, 384, 70, 28, 28, 11, DG_MAX_NEG + 1, 0), make_desc(2, 8200, 70, 28, 28, 11, 1, 0), make_desc(2, 384, 129, 28, 28, 11, 1, 0),
            make_desc(2, 384, 70, 129, 128, 11, 1, 0), make_desc(2, 384, 70, 28, 28, 11, 1, 0, 14, 0), make_desc(2, 384, 70, 28, 28, 11, 1, 0, -1, -1),
            make_desc(2, 384, 70, 28, 28, 11, 1, 0, 129, 128), make_desc(2, 1024, 70, 28, 28, 14, 1, 0), make_desc(2, 1024, 70, 28, 28, 28, 1, DENSE),
            make_desc(2, 384, 70, 28, 28, 11, 1, DG_FEATS_UNIT), make_desc(2, 384, 70, 28, 28, 28, 1, DG_IDENTITY_GRID),
            make_desc(2, 384, 70, 28, 28, 14, 1, DENSE), make_desc(2, 384, 70, 28, 30, 28, 1, DENSE), make_desc(1, 384, 70, 72, 72, 72, 1, DENSE),
            make_desc(2, 384, 70, 28, 28, 28, 1, DENSE | DG_LINE_GRID), make_desc(2, 384, 70, 28, 28, 28, 1, DENSE, 14, 14),
            make_desc(8193, 384, 70, 28, 28, 11, 1, 0),          // (accepted by make_plan; the in-call draw refuses B)
        };
        for (const dg_corr_desc& d : bad) visit(&d, true, "bad");
    }
    static const int Ns[] = {0, 1, 2, DG_MAX_NEG};
    int k = 0;
    for (const Shape& s : kShapes)
        for (int bi = 0; bi < 3 && s.Bs[bi]; ++bi)
            for (int N : Ns)
                for (uint32_t bits = 0; bits < ((s.grid & DG_IDENTITY_GRID) ? 128u : 64u); ++bits) {
                    uint32_t f = s.grid;
                    if (bits & 1) f |= DG_POINTWISE;
                    if (bits & 2) f |= DG_ZERO_CLAMP;
                    if (bits & 4) f |= DG_STABALIZE;
                    if (bits & 8) f |= DG_DEPTH_TERM;
                    if (bits & 16) f |= DG_NEED_GRAD;
                    if (bits & 32) f |= DG_EXACT_MASKS;
                    if (bits & 64) f |= DG_FEATS_UNIT;
                    const dg_corr_desc d = make_desc(s.Bs[bi], s.C, s.D, s.h, s.w, s.S, N, f, s.ch, s.cw);
                    visit(&d, k++ % 8 == 0);
                }
    // the measurement aid's span pointer rides in the fused launches' argument blocks
    {
        dg_prof_main_span(fake<void>(0x320000000000ull));
        const dg_corr_desc d1 = make_desc(8, 384, 70, 28, 28, 28, 2, DENSE | DG_POINTWISE | DG_ZERO_CLAMP | DG_NEED_GRAD | DG_DEPTH_TERM);
        const dg_corr_desc d2 = make_desc(8, 384, 70, 28, 28, 11, 2, DG_POINTWISE | DG_ZERO_CLAMP | DG_NEED_GRAD);
        visit(&d1, false, "span"); visit(&d2, false, "span");
        dg_prof_main_span(nullptr);
    }
    // the two stand-alone launches of the unit
    {
        const dg_corr_desc* d = nullptr;
        float* dst[3] = {fake<float>(0x330000000000ull), fake<float>(0x340000000000ull), fake<float>(0x350000000000ull)};
        CALL(dg_sampled_sumsq, 4, 1024, 28, 28, 14, 0, FEATS, COORDS1, PERMS, 1, OUT, CALLER);
        CALL(dg_sampled_sumsq, 4, 1024, 28, 28, 14, 1, FEATS, COORDS1, nullptr, 0, OUT, CALLER);
        CALL(dg_sampled_sumsq, 4, 1024, 28, 28, 14, 1, nullptr, COORDS1, nullptr, 0, OUT, CALLER);
        CALL(dg_normalize_split, 4, 1024, 28, 28, FEATS, 3, 384, dst, CALLER);
        CALL(dg_normalize_split, 4, 1024, 28, 28, FEATS, 2, 384, dst, CALLER);
        dst[1] = nullptr;
        CALL(dg_normalize_split, 4, 1024, 28, 28, FEATS, 3, 384, dst, CALLER);
    }
    // every launcher (and the two event calls) failing in turn, on one descriptor of every preparation route
    {
        const uint32_t full = DG_POINTWISE | DG_ZERO_CLAMP | DG_NEED_GRAD | DG_DEPTH_TERM;
        const dg_corr_desc fd[] = {
            make_desc(8, 384, 70, 28, 28, 28, 2, DENSE | full | DG_EXACT_MASKS), make_desc(8, 384, 70, 28, 28, 28, 2, DENSE | DG_ZERO_CLAMP | DG_NEED_GRAD | DG_DEPTH_TERM | DG_EXACT_MASKS),
            make_desc(8, 384, 70, 28, 28, 28, 1, DENSE | DG_POINTWISE | DG_DEPTH_TERM), make_desc(4, 384, 70, 28, 28, 12, 2, full),
            make_desc(2, 384, 70, 40, 40, 12, 1, full), make_desc(3, 384, 70, 28, 28, 14, 2, full), make_desc(2, 768, 70, 28, 28, 14, 1, full),
            make_desc(2, 384, 70, 40, 40, 20, 1, DG_POINTWISE | DG_NEED_GRAD | DG_DEPTH_TERM)};
        static const char* const names[] = {"dg_launch_corr", "dg_launch_corr2", "dg_launch_gs", "dg_launch_finish", "dg_launch_transpose", "dg_launch_gather",
            "dg_launch_cd_mask", "dg_launch_cd_mask3", "dg_launch_plane_sample", "dg_launch_colmean", "dg_launch_prep_dense", "dg_launch_rowmean",
            "dg_launch_set_stash", "dg_launch_scatter", "dg_launch_pre_general", "dg_launch_corr_small", "dg_launch_small_finish", "dg_launch_gather_rows",
            "dg_launch_cd_hist", "hipMemsetAsync", "hipEventRecord", "hipStreamWaitEvent"};
        for (const char* n : names)
            for (const dg_corr_desc& d : fd) { g_fail_name = n; visit(&d, false, n); }
        g_fail_name.clear();
    }
    if (g_only >= 0) return 0;
    for (const auto& t : g_main_texts) printf("note: failed fused launch, %ld calls: %s\n", t.second, t.first.c_str());
    printf("descriptors=%d calls=%ld launches=%ld digest=%016llx\n", g_index, g_calls, g_launches, (unsigned long long)g_hash);
    for (const auto& r : g_routes) printf("route %s %ld\n", r.first.c_str(), r.second);

    // every route the grid has to reach; the two switches each trade one route for another
    const char* e;
    const bool fold_off = (e = getenv("DG_FOLD_INTRA")) && e[0] == '0', split_off = (e = getenv("DG_SPLIT_MASKS")) && e[0] == '0';
    std::vector<std::string> need = {
        "small_nsplit1", "small_nsplit2", "small_plane_sampler", "small_gather_code_maps_of_another_size", "small_gather_maps_above_1024_pixels",
        "general_blobs", "general_S14plus", "general_line_grid", "general_plane_sampler", "general_channel_last", "rf4", "rf8",
        "dense_pointwise", "dense_plain", "dense_exact_raw", "dense_exact_split", "dense_sign_masks", "exact_masks_small_sample_grid",
        "half", "grouped", "grouped_28x28_shared", "grouped_B8", "grouped_B64", "grouped_N1", "grouped_N2plus",
        "grad_k_corr2", "grad_k_corr_main", "depth_as_job", "depth_as_gs_blocks", "masked_depth_side_stream", "masked_depth_caller_stream",
        "n_neg_0", "n_neg_1", "n_neg_max", "KF128", "KF384", "KF768", "KD96", "KD128", "stabalize", "no_zero_clamp",
        "feat_inv", "feat_keep", "draw_with_state", "draw_without_state", "refused", "launch_failed", "materialize_depth", "materialize_pairset",
        "backward_small_merged", "backward_dense", "backward_general", "xop",
        "entry_dg_corr_workspace_bytes", "entry_dg_corr_forward", "entry_dg_corr_forward_extnorm", "entry_dg_corr_forward_draw",
        "entry_dg_corr_forward_masked", "entry_dg_corr_workspace_bytes_intra_feats", "entry_dg_corr_forward_intra_feats", "entry_dg_corr_backward", "entry_dg_corr_backward_total", "entry_dg_corr_materialize",
        "entry_dg_corr_materialize_shared", "entry_dg_corr_cd_hist", "entry_dg_corr_relaunch_main", "entry_dg_corr_intra_folded", "entry_dg_corr_main_kernel_name"};
    need.push_back(fold_off ? "pointwise_k_corr2_unfolded" : "fold");
    if (!fold_off) need.push_back("materialize_after_fold");
    need.push_back(split_off ? "mask3_caller_stream_with_side" : "mask3_side_stream");
    need.push_back("mask3_caller_stream_no_side");
    int missing = 0;
    for (const std::string& r : need) if (!g_routes.count(r)) { fprintf(stderr, "route not reached: %s\n", r.c_str()); ++missing; }
    printf("note: dg_launch_corr2 was asked %ld times for a launch it does not support\n", g_corr2_declined);
    if (g_mismatch) fprintf(stderr, "%d kernel-name mismatches\n", g_mismatch);
    return (missing || g_mismatch) ? 1 : 0;
}
