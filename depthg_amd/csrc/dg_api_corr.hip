// C ABI of the gfx950 DepthG library (include/depthg_corr.h): the correlation loss.  Host-side orchestration only: workspace
// carving (Plan), job tables, kernel launches on the caller's stream and the library's side stream.
#include "dg_api.h"
#include "dg_corr_args.h"
#include "dg_taps.h"          // dg_taps_record_bytes

// ---- measurement aid: the fused correlation launch's execution span (include/depthg_corr.h dg_prof_main_span)
static unsigned long long* g_prof_span = nullptr;
extern "C" int dg_prof_main_span(void* span) { g_prof_span = static_cast<unsigned long long*>(span); return DG_OK; }

// ---- the plan: everything that decides which kernels a call runs, on which operands and from which workspace regions, decided ONCE
// per descriptor by make_plan.  Every job builder and every launch below reads it; none of them derives a route again.
enum class Prep { Small, Dense, General };              // operand preparation: the fused small grid (dg_small.hip: sampled rows -> ONE launch) /
                                                        // the dense identity grid straight from NCHW / general coordinates into blobs
enum class Sampler { Plane, ChannelLast, Direct };      // sample(): k_plane_sample straight from NCHW / channel-last copies of the maps + a gather /
                                                        // k_sample_direct: the four taps read in place (feature maps above 16384 positions)
enum class MainKernel { Small, Corr2, CorrMain };       // the fused correlation launch: k_corr_small / k_corr2 (gradient passes of the
                                                        // shapes dg_corr2_shape_supported names) / k_corr_main (everything else)
enum class Depth { None, Job, GsBlocks, GsOwnLaunch };   // the depth term of the blob kernels: off (or inside k_corr_small) / a job of the fused launch
                                                        // (forward-only calls) / blocks of the k_gs launch (gradient passes; dg_corr.hip gs_depth_block: in
                                                        // the fused kernel's launch its latency-bound blocks were the tail) / those blocks, in the masked
                                                        // form, as a launch of their own beside the G-stream blocks (fwd_finish)
enum class Hist { Rows, Blobs };                          // dg_corr_cd_hist: the sampled fp32 code rows of the fused small grid (k_cd_hist_rows) / the
                                                        // fp16 C parts of the operand blobs (k_cd_hist)
enum class Masks { None, Sampled, DenseRaw, DenseSplit };   // exact clamp masks: the sign of the fp16 cd / k_cd_mask blocks inside the gather launch
                                                        // (small sample grids) / k_cd_mask on channel-last code maps / k_cd_mask3 on split fp16 operands

struct PairSet {            // pair-set t: 0 intra, 1 inter, 2 + k negative k
    int rop;                // the stationary operand: operand 0 - but for the intra pair-set of dg_corr_forward_intra_feats, whose two sides
                            // are both the intra feature operand (Plan::xop)
    int op;                 // the streamed operand (pass A)
    int neg;                // k, or -1
    bool mapped;            // the streamed operand is read through negative k's batch map (DG_SHARED_COORDS: the negatives stream operand 0)
    float shift;
    int slot_loss, slot_cd; // DG_OUT_*
    float fin_scale;        // 1 / numel of the tensor the pair-set's sums are means of
    int gidx, csel, dest;   // the backward: upstream scalar, coordinate set and destination map of the streamed-side gradient ...
    float factor;           // ... and the constant factor of both sides
};
struct Operand {            // operand o: 0 anchors, 1 positives, 2 + k the negatives' (not with DG_SHARED_COORDS)
    int srcsel;             // 1: the *_pos maps (operand 1); 0: orig_feats / orig_code
    int cset;               // 0: coords1, 1: coords2
    int map;                // k: read through negative k's batch map; -1: none
};

struct Plan {
    int B, C, D, h, w, hc, wc, S, Sh, P, Ppad, KF, KD, C4, D4, N, T, nops, rf, nrb;     // (hc, wc): size of the code maps
    bool shared, depth, grad, pointwise;
    // dg_corr_forward_intra_feats: operand xop = T (-1: none) is one more prepared operand - intra_feats sampled at coords1 as its F
    // part (rows), operand 0's code as its C part (the code rows ARE operand 0's: rows_c[xop] == rows_c[0]) - and both sides of
    // pair-set 0.  Its regions lie behind everything the plain plan lays out, whose offsets are the same with and without it: the
    // backward, dg_corr_cd_hist and dg_corr_materialize plan from the descriptor alone and find what they read (gradient tiles, code
    // rows, C parts and inverse norms of operand 0, tap records) where the forward left it.
    int xop;
    size_t nhwc_x;
    int nopx() const { return nops + (xop >= 0 ? 1 : 0); }       // prepared operands
    // ---- routes
    Prep prep;
    Sampler sampler;                        // (Prep::Dense samples nothing: ChannelLast, the copies its DenseRaw masks read)
    MainKernel main;
    Masks masks;
    Hist hist;
    bool fold;                              // MainKernel::Corr2 forms the intra pair-set's streamed-side gradient itself (dg_corr2.hip FOLD)
    bool half;                              // MainKernel::Corr2 and k_gs write fp16 gradient tiles for k_combine_out (identity grid; DgScatterSrc.half)
    Depth depth_run;
    int nsplit;                             // Prep::Small: blocks per (image, pair-set), 2 when the image has 5 tiles
    int dep_nrb;                            // row blocks of the depth term inside the k_gs launch: 8 row tiles each
    float lo, hi;                           // clamp bounds of cd (zero_clamp / stabalize)
    float shift_depth;
    float inv_numel;                        // 1 / (B P P)
    float grad_f, grad_fn;                  // the backward's factors: -1 / (B P P) (the kernels keep -G: the sign lives here), and / n_neg
    int blob, blob_off_c;                   // the operand blobs at (KF, KD): bytes per tile, offset of the C part (DgBlob)
    PairSet ps[DG_MAX_NEG + 2];
    Operand ops[DG_MAX_NEG + 2];
    // Ragged last row blocks grouped by streamed operand (dg_corr2.hip): pair-sets that stream the same operand form a key.  Worth it
    // when the ragged row block is short (at most 4 of the 8 row tiles) and several pair-sets share an operand (shared coordinates:
    // intra + the negatives stream operand 0 through batch maps).  gr_on: in use; key and first are filled whenever the shape is eligible
    bool gr_on;
    int gr_nkeys, gr_cpb, gr_blocks_per_image;
    int8_t gr_key[DG_MAX_JOBS], gr_first[DG_MAX_JOBS];
    int32_t gr_nblk[DG_MAX_JOBS];
    // ---- workspace offsets
    size_t nhwc_f[2], nhwc_c[2];
    size_t rows_f[DG_MAX_NEG + 2], rows_c[DG_MAX_NEG + 2];     // sampled fp32 rows per operand (small sample grids)
    size_t op[DG_MAX_NEG + 2], inv[DG_MAX_NEG + 2], colpart[DG_MAX_NEG + 2], bbar[DG_MAX_NEG + 2];
    size_t ccolpart[DG_MAX_NEG + 2], csum[DG_MAX_NEG + 2], bsplit[DG_MAX_NEG + 2];
    size_t rvec[DG_MAX_NEG + 2], rimg[DG_MAX_NEG + 2];
    size_t nz, nzsum;
    size_t dRA[DG_MAX_NEG + 3], dRB[DG_MAX_NEG + 2];   // dRA[T] = depth job
    size_t part[DG_MAX_NEG + 3];
    size_t comb[2], scratch_out, taps, gbuf[DG_MAX_NEG + 2];
    size_t ticket;                          // the depth blocks' ticket of the k_gs launch
    size_t maskbits[DG_MAX_NEG + 2];        // exact clamp masks of the pair-sets
    size_t clo[2];                          // Masks::DenseSplit: the parts of the normalised code the fp16 C parts drop (k_cd_mask3)
    size_t gr_list, gr_count, gr_rank;      // consumer lists of the grouped ragged row blocks
    size_t dRA2[DG_MAX_NEG + 2], dRBs[DG_MAX_NEG + 2], dRB2[DG_MAX_NEG + 2][2], dRBm[DG_MAX_NEG + 2], part4, om;      // Prep::Small
    size_t total;

    bool small() const { return prep == Prep::Small; }
    bool dense() const { return prep == Prep::Dense; }
    bool plane() const { return sampler == Sampler::Plane; }
    bool direct() const { return sampler == Sampler::Direct; }
    bool sampled_rows() const { return sampler != Sampler::ChannelLast; }      // the sampler itself leaves rows per operand (batch maps applied)
    bool has_masks() const { return masks != Masks::None; }
    bool depth_in_gs() const { return depth_run == Depth::GsBlocks || depth_run == Depth::GsOwnLaunch; }
    bool dense_masks() const { return masks == Masks::DenseRaw || masks == Masks::DenseSplit; }
    // Without `pointwise` the intra pair-set (t = 0) has NO k_gs job (round 4): it correlates the anchors with themselves at the same
    // coordinates, so fd, cd and with them -G are symmetric and the gradient through the streamed side equals the one through the
    // stationary side, which the fused kernel accumulates in registers anyway - the backward doubles that one (as it always did for the
    // depth term) instead of reading 1/7 of the G tiles again.  With `pointwise` -G is NOT symmetric: the reference centres fd by its
    // ROW means only (fd -= fd.mean([3, 4]), src/modules.py:1238-1239), -G[p][q] - -G[q][p] = mask (rowmean_q - rowmean_p) - invisible
    // on i.i.d. features, 1e-2 of the gradient on the FPS recipes (the test with exact masks caught it).
    // (fold: with `pointwise` k_corr2 forms G + G^T in its own accumulator, dg_corr2.hip FOLD - the same consequence for the launches)
    bool intra_symmetric() const { return !pointwise || fold; }
    // the batch map pair-set t / operand o reads its streamed images through (null: the image itself).  Formed as an integer: where no
    // mapped pair-set is read (dg_corr_materialize of intra / inter on a shared grid) `perms` may be null and the address is never used
    const int64_t* batch_map(int k, const int64_t* perms) const {
        return k < 0 ? nullptr : reinterpret_cast<const int64_t*>(reinterpret_cast<uintptr_t>(perms) + (size_t)k * B * sizeof(int64_t));
    }
    const int64_t* map_of(int t, const int64_t* perms) const { return batch_map(ps[t].mapped ? ps[t].neg : -1, perms); }
};

static inline float* f32(char* ws, size_t off) { return reinterpret_cast<float*>(ws + off); }

#define DG_CHANNEL_LAST_MAX_POS 16384    // positions of a map the channel-last route copies (feature maps above it: Sampler::Direct; code maps: refused)
#define FOLD_STASH_OFF (5 * 1024)        // k_corr2<24, 6, 5>: code k-step 5 of the C part (channels 80 .. 95: padding for D <= 80)

// the pair-set and operand tables, and from them the grouping of the ragged row blocks
static void plan_tables(const dg_corr_desc* d, Plan& p) {
    const double numel = (double)p.B * p.P * p.P;
    p.inv_numel = (float)(1.0 / numel);
    p.grad_f = (float)(-1.0 / numel);
    p.grad_fn = p.N > 0 ? p.grad_f / (float)p.N : 0.f;
    for (int t = 0; t < p.T; ++t) {
        PairSet& s = p.ps[t];
        const bool neg = t >= 2;
        s.neg = neg ? t - 2 : -1;
        s.mapped = neg && p.shared;
        s.op = s.mapped ? 0 : t;
        s.rop = 0;
        if (t == 0 && p.xop >= 0) s.op = s.rop = p.xop;
        s.shift = t == 0 ? d->shift_intra : (t == 1 ? d->shift_inter : d->shift_neg);
        s.slot_loss = neg ? DG_OUT_LOSS_NEG : t;
        s.slot_cd = neg ? DG_OUT_CD_NEG : DG_OUT_CD_INTRA + t;
        s.fin_scale = neg ? (float)(1.0 / (numel * p.N)) : p.inv_numel;
        s.gidx = neg ? 2 : t; s.csel = t == 0 ? 0 : 1; s.dest = t == 1 ? 1 : 0;
        s.factor = neg ? p.grad_fn : p.grad_f;
    }
    for (int o = 0; o < p.nops; ++o) p.ops[o] = Operand{o == 1 ? 1 : 0, o == 0 ? 0 : 1, o >= 2 ? o - 2 : -1};
    if (p.xop >= 0) p.ops[p.xop] = Operand{0, 0, -1};       // (srcsel: of its CODE; its features are intra_feats)
    const int L = (p.Ppad / 32) % 8;        // row tiles of the ragged last row block
    if (!(p.grad && p.KF == 384 && p.KD == 96 && p.D <= 80 && p.nrb > 1 && L >= 1 && L <= 4 && p.B % 8 == 0 && p.B <= 64)) return;
    int nkeys = 0, members[DG_MAX_JOBS] = {0};
    for (int t = 0; t < p.T; ++t) {
        int k = -1;
        for (int q = 0; q < nkeys; ++q) if (p.ps[p.gr_first[q]].op == p.ps[t].op) k = q;
        if (k < 0) { k = nkeys++; p.gr_first[k] = (int8_t)t; }
        p.gr_key[t] = (int8_t)k; ++members[k];
    }
    for (int k = 0; k < nkeys; ++k) p.gr_on |= members[k] > 1;
    if (!p.gr_on) return;
    p.gr_nkeys = nkeys; p.gr_cpb = 8 / L;
    for (int k = 0; k < nkeys; ++k) {
        const bool single = members[k] == 1 && !p.ps[p.gr_first[k]].mapped;             // exactly one consumer per image
        const int nb = single ? 1 : (5 * members[k] / 2 + p.gr_cpb - 1) / p.gr_cpb;     // 2.5 x the mean consumer count
        const int cap = (DG_GR_CAP + p.gr_cpb - 1) / p.gr_cpb;
        p.gr_nblk[k] = nb > cap ? cap : nb;
        p.gr_blocks_per_image += p.gr_nblk[k];
    }
}

static int make_plan(const dg_corr_desc* d, Plan& p, bool intra_feats = false) {
    if (!d) return fail(DG_ERR_INVALID, "null descriptor");
    p.xop = -1;
    if (intra_feats) {
        // what dg_corr_forward_intra_feats serves: the coordinates DepthContrastiveCorrelationLoss draws (random or salience, per
        // image, src/modules.py:1415-1425) and its six-tuple (no depth term, :1458-1463)
        if (d->flags & DG_IDENTITY_GRID) return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: DG_IDENTITY_GRID is not served (general coordinates only)");
        if (d->flags & DG_SHARED_COORDS) return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: DG_SHARED_COORDS is not served (coordinates per image only)");
        if (d->flags & DG_LINE_GRID) return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: DG_LINE_GRID is not served (the class draws S x S grids)");
        if (d->flags & DG_DEPTH_TERM) return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: DG_DEPTH_TERM is not served (the class has no depth term)");
        if ((d->code_h || d->code_w) && (d->code_h != d->h || d->code_w != d->w))
            return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: code maps of %dx%d against feature maps of %dx%d are not served (one size only)",
                        d->code_h, d->code_w, d->h, d->w);
        if (d->C > 768) return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: C=%d > 768 feature channels are not served", d->C);
        if (d->n_neg > DG_MAX_NEG - 1)
            return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: n_neg=%d > %d (one operand slot holds the intra features)", d->n_neg, DG_MAX_NEG - 1);
        if (d->h > 0 && d->w > 0 && (size_t)d->h * d->w > DG_CHANNEL_LAST_MAX_POS)
            return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: feature map %dx%d too large (max %d positions)", d->h, d->w, DG_CHANNEL_LAST_MAX_POS);
    }
    if (d->B < 1 || d->C < 1 || d->D < 1 || d->h < 1 || d->w < 1 || d->S < 1)
        return fail(DG_ERR_INVALID, "non-positive dimension in descriptor");
    if (d->n_neg < 0 || d->n_neg > DG_MAX_NEG) return fail(DG_ERR_UNSUPPORTED, "n_neg=%d outside [0,%d]", d->n_neg, DG_MAX_NEG);
    if (d->C > 8192) return fail(DG_ERR_UNSUPPORTED, "C=%d > 8192 feature channels not supported", d->C);
    if (d->D > 128) return fail(DG_ERR_UNSUPPORTED, "D=%d > 128 code channels not supported", d->D);
    if ((size_t)d->h * d->w > DG_SAMPLE_DIRECT_MAX_POS)
        return fail(DG_ERR_UNSUPPORTED, "feature map %dx%d too large (max %d positions)", d->h, d->w, DG_SAMPLE_DIRECT_MAX_POS);
    if (d->code_h < 0 || d->code_w < 0 || (d->code_h == 0) != (d->code_w == 0))
        return fail(DG_ERR_INVALID, "code_h=%d, code_w=%d: both zero (code maps of the feature maps' size) or both positive", d->code_h, d->code_w);
    p.B = d->B; p.C = d->C; p.D = d->D; p.h = d->h; p.w = d->w; p.S = d->S; p.N = d->n_neg;
    p.hc = d->code_h ? d->code_h : d->h; p.wc = d->code_w ? d->code_w : d->w;
    if ((size_t)p.hc * p.wc > DG_CHANNEL_LAST_MAX_POS) return fail(DG_ERR_UNSUPPORTED, "code map %dx%d too large", p.hc, p.wc);
    const bool same_maps = p.hc == p.h && p.wc == p.w;
    p.Sh = (d->flags & DG_LINE_GRID) ? 1 : d->S;      // sample grid: Sh rows x S columns
    p.P = p.Sh * d->S;
    p.Ppad = (int)up(p.P, 32);
    p.KF = d->C <= 128 ? 128 : (d->C <= 384 ? 384 : 768);
    p.KD = d->D <= 96 ? 96 : 128;
    // Sample grids of at most 160 positions (every recipe the reference ships: feature_samples = 11 / 12) take the fused small-grid
    // kernel, which streams the feature channels in chunks and so has no width limit (FeaturePyramidNet: 2048).  The blob kernels
    // (larger grids, the identity grid) hold whole channel vectors in registers / LDS: C <= 768 there.
    const bool ident = (d->flags & DG_IDENTITY_GRID) != 0;
    p.prep = ident ? Prep::Dense : (dg_small_supported(p.Ppad, p.KD) ? Prep::Small : Prep::General);
    p.nsplit = p.Ppad == 160 ? 2 : 1;
    p.hist = p.small() ? Hist::Rows : Hist::Blobs;    // (what the forward leaves behind: the fused small grid keeps rows, every other path code blobs)
    if (d->C > 768 && !p.small())
        return fail(DG_ERR_UNSUPPORTED, "C=%d > 768 feature channels are supported on sample grids of at most 160 positions "
                                        "(feature_samples <= 12) only; this call has %d positions%s", d->C, p.P,
                    ident ? " on the dense identity grid (wider maps go there in channel chunks: dg_normalize_split + DG_FEATS_UNIT)"
                          : " (wider maps go there in channel chunks: dg_sampled_sumsq + dg_corr_forward_extnorm)");
    if ((d->flags & DG_FEATS_UNIT) && !ident)
        return fail(DG_ERR_INVALID, "DG_FEATS_UNIT needs DG_IDENTITY_GRID: on sampled coordinates the reference normalises BEHIND sample()");
    p.C4 = (int)up(d->C, 4); p.D4 = (int)up(d->D, 4);
    p.T = 2 + p.N;
    p.shared = (d->flags & DG_SHARED_COORDS) != 0;
    p.depth = (d->flags & DG_DEPTH_TERM) != 0;
    p.grad = (d->flags & DG_NEED_GRAD) != 0;
    p.pointwise = (d->flags & DG_POINTWISE) != 0;
    if (ident && (p.Sh != p.S || !p.shared || d->S != d->h || d->S != d->w || d->w > 64))
        return fail(DG_ERR_INVALID, "DG_IDENTITY_GRID needs DG_SHARED_COORDS and S == h == w <= 64");
    if (ident && !same_maps)
        return fail(DG_ERR_INVALID, "DG_IDENTITY_GRID needs code maps of the feature maps' size (got %dx%d against %dx%d)", p.hc, p.wc, p.h, p.w);
    p.nops = p.shared ? 2 : p.T;
    p.rf = (p.KF == 384 && p.KD == 96 && p.Ppad > 128) ? 8 : 4;    // waves per block (32 stationary rows each)
    p.nrb = (p.Ppad + p.rf * 32 - 1) / (p.rf * 32);
    p.dep_nrb = (p.Ppad / 32 + 7) / 8;
    { const DgBlob bl(p.KF, p.KD); p.blob = bl.bytes; p.blob_off_c = bl.off_c; }
    p.lo = (d->flags & DG_ZERO_CLAMP) ? 0.0f : -9999.0f;
    p.hi = (d->flags & DG_STABALIZE) ? 0.8f : __builtin_inff();
    p.shift_depth = d->shift_depth;
    const bool plain_zero_clamp = (d->flags & DG_ZERO_CLAMP) && !(d->flags & DG_STABALIZE);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += up(bytes, 256); return o; };
    const size_t HW = (size_t)p.h * p.w, HWc = (size_t)p.hc * p.wc, B = p.B;
    // small sample grids (all operands together sample fewer positions than the two maps have pixels; planes of 32 channels
    // fit the LDS; batch indices fit the 16-bit consumer lists): sample() straight from NCHW (k_plane_sample) instead of
    // channel-last copies of the whole maps
    // (code maps of another size than the feature maps - the FeaturePyramidNet contract - take the channel-last gather path)
    const bool rows = !ident && same_maps && (size_t)p.nops * p.P <= 2 * HW && HW <= 1024 && B <= 32767;
    // feature maps above the channel-last route's limit (cfg.use_true_labels: the signal has the labels' resolution): the taps are read
    // in place (k_sample_direct) - the sample grid touches a few percent of such a map, and a copy of it is hundreds of megabytes
    const bool direct = !ident && HW > DG_CHANNEL_LAST_MAX_POS;
    p.sampler = rows ? Sampler::Plane : (direct ? Sampler::Direct : Sampler::ChannelLast);
    if (direct && B > 65535) return fail(DG_ERR_UNSUPPORTED, "B=%d > 65535 images on a feature map above %d positions", p.B, DG_CHANNEL_LAST_MAX_POS);
    const bool copies = p.sampler == Sampler::ChannelLast;
    for (int i = 0; i < 2; ++i) { p.nhwc_f[i] = take(copies ? B * HW * p.C4 * 4 : 0); p.nhwc_c[i] = take(copies ? B * HWc * p.D4 * 4 : 0); }
    const bool want_rows = rows || direct || p.small();      // (the fused small-grid kernel reads sampled rows whichever sampler wrote them)
    // (the fused small-grid kernel takes bf16 feature rows of up(C, 128) channels - whole chunks; the multi-launch path fp32 rows of C4)
    const size_t frow = p.small() ? (size_t)up(p.C, 128) * 2 : (size_t)p.C4 * 4;
    for (int i = 0; i < p.nops; ++i) { p.rows_f[i] = take(want_rows ? B * p.P * frow : 0); p.rows_c[i] = take(want_rows ? B * p.P * p.D4 * 4 : 0); }
    for (int i = 0; i < p.nops; ++i) {
        p.op[i] = take(B * (p.Ppad / 32) * (size_t)p.blob);
        p.inv[i] = take(B * p.Ppad * 4);
        p.colpart[i] = take(B * (size_t)(ident ? p.h * ((p.w + 31) / 32) : p.Ppad / 32) * p.KF * 4);
        p.bbar[i] = take(B * p.KF * 4);
        p.bsplit[i] = take(B * 2 * p.KF * 2);
        p.ccolpart[i] = take(B * (size_t)(p.Ppad / 32) * p.KD * 4);
        p.csum[i] = take(B * p.KD * 4);
    }
    for (int t = 0; t < p.T; ++t) { p.rvec[t] = take(B * p.Ppad * 4); p.rimg[t] = take(B * 4); }
    p.nz = take(B * p.Ppad * 4);
    p.nzsum = take(B * 4);
    for (int t = 0; t <= p.T; ++t) { p.dRA[t] = take(B * p.Ppad * p.KD * 4); p.part[t] = take(B * p.nrb * 2 * 4); }
    for (int t = 0; t < p.T; ++t) p.dRB[t] = take(B * p.Ppad * p.KD * 4);
    for (int i = 0; i < 2; ++i) p.comb[i] = take(B * p.Ppad * p.KD * 4);
    p.scratch_out = take(DG_OUT_COUNT * 4);
    p.taps = take(2 * B * dg_taps_record_bytes(p.hc * p.wc, p.P));     // the adjoint of sample() scatters into the CODE maps
    for (int t = 0; t < p.T; ++t) p.gbuf[t] = p.grad ? take(B * (size_t)(p.Ppad / 32) * (p.Ppad / 32) * 2048) : 0;     // (gbuf[0]: 4 KiB would do with p.fold)
    p.ticket = take(256);
    // The mask source.  Sampled: gradient passes of the zero_clamp recipe on small sample grids (fp32 sampled rows exist, <= 8 tiles, the
    // one-wave-per-SIMD form of k_corr_main).  DG_EXACT_MASKS: the dense identity grid at the widths of the one-wave-per-SIMD kernel
    // (dg_corr2.hip) takes the same mask words - without `pointwise` from channel-last fp32 copies of the two code maps (the workspace's
    // nhwc_c regions, otherwise unused on this grid), with it from the split fp16 operands the k_colmean launch writes
    const bool xmask = rows && !p.small() && p.grad && plain_zero_clamp && p.Ppad <= 256 && p.rf == 4;
    const bool xmask_dense = (d->flags & DG_EXACT_MASKS) && ident && p.grad && plain_zero_clamp &&
                             p.KF == 384 && p.KD == 96 && p.D <= 80 && p.Ppad >= 160 && p.B <= 64;
    if ((d->flags & DG_EXACT_MASKS) && p.grad && (d->flags & DG_ZERO_CLAMP) && !xmask && !xmask_dense && !p.small())
        return fail(DG_ERR_UNSUPPORTED, "DG_EXACT_MASKS: exact clamp masks exist on small sample grids (always on there) and on the dense "
                                        "identity grid with C <= 384 (padded to 384), D <= 80, P >= 160, B <= 64, zero_clamp without stabalize");
    p.masks = xmask ? Masks::Sampled : (!xmask_dense ? Masks::None : (p.pointwise ? Masks::DenseSplit : Masks::DenseRaw));
    for (int t = 0; t < p.T; ++t) p.maskbits[t] = take(p.has_masks() ? B * (size_t)(p.Ppad / 32) * p.Ppad * 4 : 0);
    // The main kernel.  On a gradient pass every job of the fused launch is a pair-set job with operand 0 stationary, G tiles wanted, no
    // batch map on R and mask words for all pair-sets or none (build_corr_jobs), so the launcher's own predicate dg_corr2_supported
    // comes down to its shape part: the plan knows the answer, and the launcher's check is the cross-check (launch_main).
    p.main = p.small() ? MainKernel::Small
                       : (p.grad && dg_corr2_shape_supported(p.KF, p.KD, p.D, p.lo, p.hi, p.Ppad, p.B) ? MainKernel::Corr2 : MainKernel::CorrMain);
    // FOLD: gradient passes of the pointwise recipe that k_corr2 runs (with the dense grid's exact mask words too, since round 6:
    // k_corr2<.., XM, .., FOLD>); DG_FOLD_INTRA=0 keeps the k_gs job (test seam, dg_common.h)
    static const bool fold_on = [] { const char* e = getenv("DG_FOLD_INTRA"); return !(e && e[0] == '0'); }();
    p.fold = fold_on && p.main == MainKernel::Corr2 && p.pointwise && !xmask;
    // fp16 gradient tiles (round 6): the identity grid's backward is ONE launch (k_combine_out) that reads the raw tiles of k_corr2 and the
    // streamed-side tiles of k_gs once - 93 of the headline step's 1342 MB go with fp32 -> fp16 (both producers bounded: the raw tiles by
    // construction, k_gs's by leaving the division by ||c|| to the consumer).  Where k_corr2 runs and k_combine_out will (its routed list
    // holds n_neg x B entries at most 512)
    p.half = p.main == MainKernel::Corr2 && ident && p.N * p.B <= 512 && p.S == p.h && p.S == p.w;
    p.depth_run = (!p.depth || p.small()) ? Depth::None : (!p.grad ? Depth::Job : (p.dense_masks() ? Depth::GsOwnLaunch : Depth::GsBlocks));
    for (int i = 0; i < 2; ++i) p.clo[i] = take(p.masks == Masks::DenseSplit ? B * (size_t)(p.Ppad / 32) * p.KD * 64 : 0);
    p.gr_list = take((size_t)DG_MAX_JOBS * B * DG_GR_CAP * 4);
    p.gr_count = take((size_t)DG_MAX_JOBS * B * 4);
    p.gr_rank = take((size_t)DG_MAX_JOBS * B * 2);
    {
        const bool sg = p.small() && p.grad, two = sg && p.pointwise;       // two: the old_mean terms of the gradient (dg_small.hip)
        const size_t gt = B * p.Ppad * p.KD * 4;
        for (int t = 0; t < p.T; ++t) {
            p.dRA2[t] = take(two ? gt : 0);
            p.dRBs[t] = take(sg && p.nsplit == 2 ? gt : 0);
            for (int k = 0; k < 2; ++k) p.dRB2[t][k] = take(two && k < p.nsplit ? gt : 0);
            p.dRBm[t] = take(sg && t >= 2 && (p.pointwise || p.nsplit == 2) ? gt : 0);
        }
        p.part4 = take(p.small() ? (size_t)(p.T + 1) * B * p.nsplit * 16 : 0);
        p.om = take(p.small() ? (size_t)(p.T + 1) * 4 : 0);
    }
    if (intra_feats) {
        // the intra feature operand, behind everything else (Plan::xop)
        const int x = p.xop = p.T;
        p.nhwc_x = take(rows ? 0 : B * HW * p.C4 * 4);
        p.rows_f[x] = take(want_rows ? B * p.P * frow : 0); p.rows_c[x] = p.rows_c[0];
        p.op[x] = take(B * (p.Ppad / 32) * (size_t)p.blob);
        p.inv[x] = take(B * p.Ppad * 4);
        p.colpart[x] = take(B * (size_t)(p.Ppad / 32) * p.KF * 4);
        p.bbar[x] = take(B * p.KF * 4);
        p.bsplit[x] = take(B * 2 * p.KF * 2);
        p.ccolpart[x] = take(B * (size_t)(p.Ppad / 32) * p.KD * 4);
        p.csum[x] = take(B * p.KD * 4);
    }
    p.total = off;
    plan_tables(d, p);
    return DG_OK;
}

extern "C" size_t dg_corr_workspace_bytes(const dg_corr_desc* desc) {
    Plan p{};
    if (make_plan(desc, p) != DG_OK) return 0;
    return p.total;
}
extern "C" size_t dg_corr_workspace_bytes_intra_feats(const dg_corr_desc* desc) {
    Plan p{};
    if (make_plan(desc, p, true) != DG_OK) return 0;
    return p.total;
}

// Fills one helper job.  passB: the stationary operand is operand 2 of pair-set t.
static DgJob helper_job(const Plan& p, char* ws, int t, bool passB, const int64_t* perms) {
    DgJob j;
    memset(&j, 0, sizeof(j));
    const int o2 = p.ps[t].op;
    const int64_t* m2 = p.map_of(t, perms);
    const int o1 = p.ps[t].rop;
    if (!passB) {
        j.Rop = ws + p.op[o1]; j.RcInv = f32(ws, p.inv[o1]); j.ridx = nullptr;
        j.Sop = ws + p.op[o2]; j.sidx = m2;
        j.Scsum = f32(ws, p.csum[o2]);
        j.center_on_lane = 1;
    } else {
        j.Rop = ws + p.op[o2]; j.RcInv = f32(ws, p.inv[o2]); j.ridx = m2;
        j.Sop = ws + p.op[o1]; j.sidx = nullptr;
        j.center_on_lane = 0;
    }
    if (p.pointwise) { j.rvec = f32(ws, p.rvec[t]); j.rimg = f32(ws, p.rimg[t]); }
    j.shift = p.ps[t].shift;
    j.kind = DG_JOB_HELPER;
    return j;
}

static DgJob depth_job(const Plan& p, char* ws) {
    DgJob j;
    memset(&j, 0, sizeof(j));
    j.Rop = ws + p.op[0]; j.Sop = ws + p.op[0]; j.RcInv = f32(ws, p.inv[0]);
    j.nzR = f32(ws, p.nz); j.nzS = f32(ws, p.nz);
    j.shift = p.shift_depth;
    j.kind = DG_JOB_DEPTH;
    j.center_on_lane = 1;
    return j;
}

static void corr_args_base(const Plan& p, char* ws, DgCorrArgs& a) {
    memset(&a, 0, sizeof(a));
    a.B = p.B; a.P = p.P; a.Ppad = p.Ppad; a.nrb = p.nrb; a.D = p.D;
    a.lo = p.lo; a.hi = p.hi;
    a.inv_BP = 1.0f / ((float)p.B * (float)p.P);
    a.dummy = ws + p.op[0];
    a.span = g_prof_span;
    a.half_tiles = p.half ? 1 : 0;
}

// k_gs jobs: one per pair-set; the producing job of the G tiles is helper_job(t) of the fused launch (R = operand 1,
// S = operand 2 of pair-set t).  The intra pair-set has none where its -G is symmetric (Plan::intra_symmetric)
static void build_gs_jobs(const Plan& p, char* ws, const int64_t* perms, DgGsArgs& g) {
    memset(&g, 0, sizeof(g));
    const int t0 = p.intra_symmetric() ? 1 : 0;
    g.njobs = p.T - t0; g.B = p.B; g.P = p.P; g.Ppad = p.Ppad; g.KF = p.KF; g.KD = p.KD; g.D = p.D;
    for (int t = t0; t < p.T; ++t) {
        const int o2 = p.ps[t].op;
        DgGsJob& J = g.jobs[t - t0];
        J.G = reinterpret_cast<const uint16_t*>(ws + p.gbuf[t]);
        J.Rop = ws + p.op[p.ps[t].rop]; J.ridx = nullptr;
        J.Sop = ws + p.op[o2]; J.sidx = p.map_of(t, perms);
        J.ScInv = f32(ws, p.inv[o2]);
        J.dS = f32(ws, p.dRB[t]);
    }
}

// Job table of the fused correlation launch: one job per pair-set (stationary = operand 1); on forward-only calls the cheap
// depth job last (Depth::Job).  (Stationary = operand 2 is only used by dg_corr_materialize, whose stores then run along the
// second position index.)
static void build_corr_jobs(const Plan& p, char* ws, const int64_t* perms, DgCorrArgs& a) {
    corr_args_base(p, ws, a);
    a.wctr = p.grad ? reinterpret_cast<uint32_t*>(ws + p.ticket) + 16 : nullptr;      // (behind the depth blocks' ticket word)
    int nj = 0;
    for (int t = 0; t < p.T; ++t) {
        DgJob j = helper_job(p, ws, t, false, perms);
        j.part = f32(ws, p.part[t]);
        j.dR = p.grad ? f32(ws, p.dRA[t]) : nullptr;
        // (the gradient of the streamed operand's code comes from k_gs, which consumes the G tiles these jobs store)
        j.Gout = p.grad ? reinterpret_cast<uint16_t*>(ws + p.gbuf[t]) : nullptr;
        j.fold = (p.fold && t == 0) ? 1 : 0;
        j.maskbits = p.has_masks() ? reinterpret_cast<const uint32_t*>(ws + p.maskbits[t]) : nullptr;
        j.slot_loss = p.ps[t].slot_loss; j.slot_cd = p.ps[t].slot_cd; j.fin_scale = p.ps[t].fin_scale;
        a.jobs[nj++] = j;
    }
    if (p.depth_run == Depth::Job) {
        DgJob j = depth_job(p, ws);
        j.part = f32(ws, p.part[p.T]);
        j.dR = nullptr;
        j.slot_loss = DG_OUT_LOSS_DEPTH; j.slot_cd = -1; j.fin_scale = p.inv_numel;
        a.jobs[nj++] = j;
    }
    a.njobs = nj;
    // the grouped ragged row blocks (key and first ride along wherever the shape is eligible; the kernels read them with gr_list only)
    memcpy(a.gr_key, p.gr_key, sizeof(a.gr_key)); memcpy(a.gr_first, p.gr_first, sizeof(a.gr_first));
    if (p.gr_on) {
        a.gr_nkeys = p.gr_nkeys; a.gr_cpb = p.gr_cpb; a.gr_blocks_per_image = p.gr_blocks_per_image;
        memcpy(a.gr_nblk, p.gr_nblk, sizeof(a.gr_nblk));
        a.gr_list = reinterpret_cast<const int32_t*>(ws + p.gr_list);
        a.gr_count = reinterpret_cast<const int32_t*>(ws + p.gr_count);
        a.gr_rank = reinterpret_cast<const int16_t*>(ws + p.gr_rank);
    }
}

// Fused correlation launch: the kernel the plan names.  dg_launch_corr2 checks its own predicate once more (dg_corr2_supported):
// a refusal there means the plan and the launcher disagree - an internal error, not a reason to run another kernel.
static int launch_main(const Plan& p, const DgCorrArgs& a, hipStream_t stream) {
    if (p.main == MainKernel::Corr2) {
        const hipError_t e = dg_launch_corr2(a, p.KF, p.KD, stream);      // the pair-set jobs, one launch
        if (e == hipErrorNotSupported) return fail(DG_ERR_LAUNCH, "internal: the plan chose k_corr2 for a launch dg_corr2_supported refuses");
        if (e != hipSuccess) return fail(DG_ERR_LAUNCH, "%s failed: %s", "dg_launch_corr2(a, p.KF, p.KD, stream)", hipGetErrorString(e));
        return DG_OK;
    }
    DG_HIP(dg_launch_corr(a, p.KF, p.KD, p.rf, p.grad ? 1 : 0, stream));
    return DG_OK;
}

struct DrawArgs { int64_t* out; uint64_t seed; unsigned long long* state; };

// (DG_SPLIT_MASKS=0: the exact-mask chain of the dense grid in sequence on the caller's stream; test seam, dg_common.h)
static bool split_masks_enabled() {
    static const bool on = [] { const char* e = getenv("DG_SPLIT_MASKS"); return !(e && e[0] == '0'); }();
    return on;
}

// the argument block of the fused small-grid kernel (dg_small.hip): forward, materialize and relaunch
static void small_args(const Plan& p, const dg_corr_desc* d, char* ws, const int64_t* perms, DgSmallArgs& a) {
    memset(&a, 0, sizeof(a));
    for (int o = 0; o < p.nopx(); ++o) { a.rowsF[o] = f32(ws, p.rows_f[o]); a.rowsC[o] = f32(ws, p.rows_c[o]); }
    a.T = p.T; a.B = p.B; a.P = p.P; a.Ppad = p.Ppad; a.C4 = (int)up(p.C, 128); a.D = p.D; a.D4 = p.D4; a.KD = p.KD;
    a.pointwise = p.pointwise ? 1 : 0; a.depth = p.depth ? 1 : 0; a.grad = p.grad ? 1 : 0;
    a.lo = p.lo; a.hi = p.hi;
    for (int t = 0; t < p.T; ++t) { a.shift[t] = p.ps[t].shift; a.opR[t] = p.ps[t].rop; a.opS[t] = p.ps[t].op; a.sidx[t] = p.map_of(t, perms); }
    a.shift_depth = p.shift_depth;
    a.nz = f32(ws, p.nz); a.nzsum = f32(ws, p.nzsum);
    for (int t = 0; t <= p.T; ++t) a.dRA[t] = f32(ws, p.dRA[t]);
    for (int t = 0; t < p.T; ++t) {
        a.dRA2[t] = f32(ws, p.dRA2[t]);
        a.dRB[t][0] = f32(ws, p.dRB[t]); a.dRB[t][1] = f32(ws, p.dRBs[t]);
        a.dRB2[t][0] = f32(ws, p.dRB2[t][0]); a.dRB2[t][1] = f32(ws, p.dRB2[t][1]);
    }
    a.part = f32(ws, p.part4); a.om = f32(ws, p.om);
    a.ticket = reinterpret_cast<unsigned int*>(ws + p.ticket) + 32;
    a.xop = ws + p.op[0]; a.xinv = f32(ws, p.inv[0]); a.blob_bytes = p.blob; a.blob_off_c = p.blob_off_c;
    a.wtot[0] = d->w_intra; a.wtot[1] = d->w_inter; a.wtot[2] = d->w_neg; a.wtot[3] = d->w_depth;
    a.nsplit = p.nsplit;
    a.span = g_prof_span;
#ifdef DG_DEVTOOLS
    { static const int dbg = [] { const char* e = getenv("DG_SMALL_DEBUG"); return e ? atoi(e) : 0; }(); a.debug = dbg; }
#endif
}

struct FeatKeep { const float* keep[2]; float scale; };      // deferred Dropout2d of the two feature maps (dg_corr_forward_masked)

// ---- the forward call: what an entry point hands in (the seven maps, the batch maps, then one extra at most) ...
struct FwdInputs {
    const float *feats, *feats_pos, *code, *code_pos, *depth, *coords1, *coords2;
    const int64_t* perms;
    const DrawArgs* draw = nullptr;     // the call draws `perms` itself
    const FeatKeep* fk = nullptr;       // dg_corr_forward_masked
    const float* feat_inv = nullptr;    // dg_corr_forward_extnorm
    const float* intra = nullptr;       // dg_corr_forward_intra_feats (intra_entry): the map behind operand p.xop's features
    bool intra_entry = false;
};

// ... and what its stages share
struct Fwd : FwdInputs {
    explicit Fwd(const FwdInputs& in) : FwdInputs(in) {}
    Plan p{};
    const dg_corr_desc* desc;
    float* out;
    char* ws; hipStream_t stream;
    // (the region object - it holds the side stream's lock - exists only on calls that use it: the exact-mask chain of the dense grid
    //  under `split`, and the k_gs launches, which re-use it)
    std::optional<SideRegion> side;
    bool split;
    DgCorrArgs a;                       // the job table of step 4 (build_corr_jobs): steps 3 and 5 read it
    const float* coords(int o) const { return p.ops[o].cset ? coords2 : coords1; }
    const int64_t* op_map(int o) const { return p.batch_map(p.ops[o].map, perms); }
};

static int fwd_validate(Fwd& c, void* workspace, size_t workspace_bytes) {
    const Plan& p = c.p;
    if (c.feat_inv && p.prep != Prep::General)
        return fail(DG_ERR_INVALID, "dg_corr_forward_extnorm is the sampled-coordinate path above 160 positions: the identity grid takes "
                                    "DG_FEATS_UNIT, smaller grids any width as they are");
    if (p.xop >= 0 && !c.intra) return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_intra_feats: intra_feats is null");
    if (c.fk && (c.fk->keep[0] || c.fk->keep[1]) && !p.dense())
        return fail(DG_ERR_UNSUPPORTED, "deferred feature dropout (feat_keep) is built for the identity grid only: "
                                        "with sampled coordinates hand the dropped features in");
    if (!c.feats || !c.feats_pos || !c.code || !c.code_pos || !c.coords1 || !c.coords2 || !c.out || !workspace)
        return fail(DG_ERR_INVALID, "null tensor pointer");
    if (p.N > 0 && !c.perms) return fail(DG_ERR_INVALID, "perms is null with n_neg=%d", p.N);
    if (p.depth && (!c.depth || c.desc->depth_h < 1 || c.desc->depth_w < 1))
        return fail(DG_ERR_INVALID, "DG_DEPTH_TERM set but depth is missing (the reference raises on depth=None too)");
    if (workspace_bytes < p.total) return fail(DG_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, p.total);
    c.ws = static_cast<char*>(workspace);
    return DG_OK;
}

// ---- table fills that more than one route of the forward shares
// The jobs that depend on nothing but the call's inputs: the draw of the batch maps, the depth indicators and, on gradient passes, the
// inverse tap records of the sample() adjoint (dg_corr_backward then finds them in the workspace)
static int pre_args(const Fwd& c, DgPreArgs& q) {
    const Plan& p = c.p;
    memset(&q, 0, sizeof(q));
    if (c.draw && p.N > 0) { q.seed = c.draw->seed; q.state = c.draw->state; q.perms = c.draw->out; q.count = p.N; }
    if (p.depth) { q.depth = c.depth; q.nz = f32(c.ws, p.nz); q.nzsum = f32(c.ws, p.nzsum); q.dH = c.desc->depth_h; q.dW = c.desc->depth_w; }
    if (p.grad && (size_t)p.hc * p.wc <= 4096 && p.P <= 65535) { q.coords1 = c.coords1; q.coords2 = c.coords2; q.taps = c.ws + p.taps; }
    q.B = p.B; q.h = p.hc; q.w = p.wc; q.S = p.S; q.Sh = p.Sh; q.P = p.P; q.Ppad = p.Ppad;      // (h, w): the maps the tap records index = the code maps
    if (p.B > 8192 && q.count > 0) return fail(DG_ERR_UNSUPPORTED, "B=%d too large for the in-call draw", p.B);
    return DG_OK;
}

// sample() straight from NCHW into rows per operand (Sampler::Plane); bf16_rows: feature rows as the fused small-grid kernel takes them
static int plane_sample(const Fwd& c, bool bf16_rows) {
    const Plan& p = c.p;
    DgPlaneArgs t;
    memset(&t, 0, sizeof(t));
    t.src[0] = c.feats; t.src[1] = c.feats_pos; t.src[2] = c.code; t.src[3] = c.code_pos;
    t.K[0] = t.K[1] = p.C; t.K4[0] = t.K4[1] = bf16_rows ? (int)up(p.C, 128) : p.C4; t.K[2] = t.K[3] = p.D; t.K4[2] = t.K4[3] = p.D4;
    t.feats_bf16 = bf16_rows ? 1 : 0;
    for (int o = 0; o < p.nops; ++o) { t.rows[o][0] = f32(c.ws, p.rows_f[o]); t.rows[o][1] = f32(c.ws, p.rows_c[o]); }
    t.coords1 = c.coords1; t.coords2 = c.coords2; t.perms = c.perms;
    t.nops = p.nops; t.B = p.B; t.h = p.h; t.w = p.w; t.S = p.S; t.Sh = p.Sh; t.P = p.P;
    if (p.xop >= 0) { t.src_x = c.intra; t.rows_x = f32(c.ws, p.rows_f[p.xop]); }
    DG_HIP(dg_launch_plane_sample(t, c.stream));
    return DG_OK;
}

// sample() with the taps read in place (Sampler::Direct): rows per operand as plane_sample leaves them, the code maps - of their own
// size - as further jobs of the one launch
static int direct_sample(const Fwd& c, bool bf16_rows) {
    const Plan& p = c.p;
    DgSampleDirectArgs g;
    memset(&g, 0, sizeof(g));
    int nj = 0;
    for (int o = 0; o < p.nops; ++o) {
        const int srcsel = p.ops[o].srcsel;
        g.src[nj] = srcsel ? c.feats_pos : c.feats; g.coords[nj] = c.coords(o); g.srcidx[nj] = c.op_map(o); g.rows[nj] = f32(c.ws, p.rows_f[o]);
        g.K[nj] = p.C; g.Kout[nj] = bf16_rows ? (int)up(p.C, 128) : p.C4; g.as_bf16[nj] = bf16_rows ? 1 : 0; g.h[nj] = p.h; g.w[nj] = p.w; ++nj;
        g.src[nj] = srcsel ? c.code_pos : c.code; g.coords[nj] = c.coords(o); g.srcidx[nj] = c.op_map(o); g.rows[nj] = f32(c.ws, p.rows_c[o]);
        g.K[nj] = p.D; g.Kout[nj] = p.D4; g.as_bf16[nj] = 0; g.h[nj] = p.hc; g.w[nj] = p.wc; ++nj;
    }
    g.njobs = nj; g.B = p.B; g.S = p.S; g.Sh = p.Sh; g.P = p.P;
    DG_HIP(dg_launch_sample_direct(g, c.stream));
    return DG_OK;
}

// channel-last copies of the four maps (the gathers read whole channel vectors per tap)
static int transpose_maps(const Fwd& c) {
    const Plan& p = c.p;
    DgTransposeArgs t;
    memset(&t, 0, sizeof(t));
    t.nmaps = 4;
    t.src[0] = c.feats; t.dst[0] = f32(c.ws, p.nhwc_f[0]); t.K[0] = p.C; t.K4[0] = p.C4; t.HW[0] = p.h * p.w;
    t.src[1] = c.feats_pos; t.dst[1] = f32(c.ws, p.nhwc_f[1]); t.K[1] = p.C; t.K4[1] = p.C4; t.HW[1] = p.h * p.w;
    t.src[2] = c.code; t.dst[2] = f32(c.ws, p.nhwc_c[0]); t.K[2] = p.D; t.K4[2] = p.D4; t.HW[2] = p.hc * p.wc;
    t.src[3] = c.code_pos; t.dst[3] = f32(c.ws, p.nhwc_c[1]); t.K[3] = p.D; t.K4[3] = p.D4; t.HW[3] = p.hc * p.wc;
    if (p.xop >= 0) { t.nmaps = 5; t.src[4] = c.intra; t.dst[4] = f32(c.ws, p.nhwc_x); t.K[4] = p.C; t.K4[4] = p.C4; t.HW[4] = p.h * p.w; }
    DG_HIP(dg_launch_transpose(t, p.B, c.stream));
    return DG_OK;
}

// exact clamp masks from fp32 code rows (k_cd_mask): rows[o] = workspace offset of operand o's rows
static void cd_mask_args(const Fwd& c, const size_t* rows, DgCdMaskArgs& m) {
    const Plan& p = c.p;
    memset(&m, 0, sizeof(m));
    m.rowsR = f32(c.ws, rows[0]);
    for (int t = 0; t < p.T; ++t) {
        m.rowsS[t] = f32(c.ws, rows[p.ps[t].op]); m.sidx[t] = p.map_of(t, c.perms);
        m.bits[t] = reinterpret_cast<uint32_t*>(c.ws + p.maskbits[t]);
    }
    m.T = p.T; m.B = p.B; m.P = p.P; m.Ppad = p.Ppad; m.D = p.D; m.D4 = p.D4;
}

// ---- the fused small-grid path (dg_small.hip)
// sampled rows of every operand (the reference's sample(), src/modules.py:822-825, of feats / code at coords1 / coords2 and of the
// negatives' permuted maps, :1323-1343) -> the fused kernel.  Launches: the draw + depth indicators + tap records, the sampler, the
// fused kernel, its one-wave finish.
static int forward_small(const Fwd& c) {
    const Plan& p = c.p;
    DgSmallArgs a;
    small_args(p, c.desc, c.ws, c.perms, a);
    a.out = c.out;
    DgPreArgs q;
    if (int rc = pre_args(c, q)) return rc;
    DG_HIP(dg_launch_pre_general(q, c.stream));
    if (p.plane()) {
        if (int rc = plane_sample(c, true)) return rc;
    } else if (p.direct()) {
        if (int rc = direct_sample(c, true)) return rc;
    } else {
        // code maps of another size than the feature maps (the FeaturePyramidNet contract) or maps beyond the plane sampler's LDS:
        // channel-last copies, then a bilinear gather into the same rows
        if (int rc = transpose_maps(c)) return rc;
        DgGatherRowsArgs g;
        memset(&g, 0, sizeof(g));
        int nj = 0;
        for (int o = 0; o < p.nops; ++o) {
            const int srcsel = p.ops[o].srcsel;
            g.src[nj] = f32(c.ws, p.nhwc_f[srcsel]); g.coords[nj] = c.coords(o); g.srcidx[nj] = c.op_map(o); g.rows[nj] = f32(c.ws, p.rows_f[o]);
            g.K4[nj] = p.C4; g.Kout[nj] = (int)up(p.C, 128); g.as_bf16[nj] = 1; g.h[nj] = p.h; g.w[nj] = p.w; ++nj;
            g.src[nj] = f32(c.ws, p.nhwc_c[srcsel]); g.coords[nj] = c.coords(o); g.srcidx[nj] = c.op_map(o); g.rows[nj] = f32(c.ws, p.rows_c[o]);
            g.K4[nj] = p.D4; g.Kout[nj] = p.D4; g.as_bf16[nj] = 0; g.h[nj] = p.hc; g.w[nj] = p.wc; ++nj;
        }
        if (p.xop >= 0) {        // the intra feature rows: one more job of this launch (the code rows are operand 0's)
            g.src[nj] = f32(c.ws, p.nhwc_x); g.coords[nj] = c.coords1; g.srcidx[nj] = nullptr; g.rows[nj] = f32(c.ws, p.rows_f[p.xop]);
            g.K4[nj] = p.C4; g.Kout[nj] = (int)up(p.C, 128); g.as_bf16[nj] = 1; g.h[nj] = p.h; g.w[nj] = p.w; ++nj;
        }
        g.njobs = nj; g.B = p.B; g.S = p.S; g.Sh = p.Sh; g.P = p.P;
        DG_HIP(dg_launch_gather_rows(g, c.stream));
    }
    DG_HIP(dg_launch_corr_small(a, c.stream));
    DG_HIP(dg_launch_small_finish(a, c.stream));
    return DG_OK;
}

// ---- the stages of the blob path (corr_forward_impl below is their driver)
// 1.+2. on the identity grid: one launch builds both feats and both code operands straight from NCHW (+ the depth indicators)
static int fwd_operands_dense(Fwd& c) {
    const Plan& p = c.p;
    DgDenseArgs g;
    memset(&g, 0, sizeof(g));
    g.src[0] = c.feats; g.src[1] = c.feats_pos; g.code[0] = c.code; g.code[1] = c.code_pos;
    for (int o = 0; o < 2; ++o) { g.blob[o] = c.ws + p.op[o]; g.colpart[o] = f32(c.ws, p.colpart[o]); g.inv_norm[o] = f32(c.ws, p.inv[o]); g.ccolpart[o] = f32(c.ws, p.ccolpart[o]); }
    g.depth = p.depth ? c.depth : nullptr; g.nz = f32(c.ws, p.nz); g.nzsum = f32(c.ws, p.nzsum);
    g.B = p.B; g.K = p.C; g.D = p.D; g.KF = p.KF; g.KD = p.KD; g.h = p.h; g.w = p.w; g.P = p.P; g.Ppad = p.Ppad;
    g.dH = c.desc->depth_h; g.dW = c.desc->depth_w;
    g.code_split = p.pointwise ? 1 : 0;        // (the code column sums then ride in the k_rowmean launch, which only pointwise has)
    g.unit = (c.desc->flags & DG_FEATS_UNIT) ? 1 : 0;
    if (c.fk) { g.fkeep[0] = c.fk->keep[0]; g.fkeep[1] = c.fk->keep[1]; g.fscale = c.fk->scale; }
    if (c.draw && p.N > 0) { g.draw_out = c.draw->out; g.draw_state = c.draw->state; g.draw_seed = c.draw->seed; g.draw_count = p.N; }
    if (c.split) {
        // the code roles (norms) and the draw on the side stream - the chain code norms -> code operands -> mask words hangs
        // off them and runs beside the feature operands, their means and the row means
        DgDenseArgs gs = g;
        gs.roles = 2 | 8; g.roles = 1 | 4;
        DG_HIP(c.side->fork());
        DG_HIP(dg_launch_prep_dense(gs, c.side->stream()));
    }
    DG_HIP(dg_launch_prep_dense(g, c.stream));
    if (p.masks == Masks::DenseRaw) {
        // exact clamp masks without `pointwise` (the code operands are then built by k_prep_dense itself, without the parts the
        // split-fp16 form of fwd_cd_mask3 needs): position-major fp32 rows of the two code maps (on this grid position p IS pixel p),
        // then the sign of every raw fp32 dot product (k_cd_mask) as one word per (S tile, R position) for all pair-sets
        DgTransposeArgs t;
        memset(&t, 0, sizeof(t));
        t.nmaps = 2;
        t.src[0] = c.code; t.dst[0] = f32(c.ws, p.nhwc_c[0]); t.K[0] = p.D; t.K4[0] = p.D4; t.HW[0] = p.h * p.w;
        t.src[1] = c.code_pos; t.dst[1] = f32(c.ws, p.nhwc_c[1]); t.K[1] = p.D; t.K4[1] = p.D4; t.HW[1] = p.h * p.w;
        DG_HIP(dg_launch_transpose(t, p.B, c.stream));
        DgCdMaskArgs m;
        cd_mask_args(c, p.nhwc_c, m);
        DG_HIP(dg_launch_cd_mask(m, c.stream));
    }
    return DG_OK;
}

// 1.+2. with general coordinates: rows per operand (k_plane_sample) or channel-last copies of the maps, then sample + normalise +
// operand blobs.  The first of these launches already reads the batch maps, so they are drawn by a launch of their own.
static int fwd_operands_general(Fwd& c) {
    const Plan& p = c.p;
    DgPreArgs q;
    if (int rc = pre_args(c, q)) return rc;
    // Nothing in front of the fused kernel reads the depth indicators or the tap records: they ride as extra blocks of the
    // gather launch below (round 4); only the draw - the sampler's first input - keeps a launch of its own
    DgPreArgs pre_late = q;
    pre_late.count = 0;
    q.depth = nullptr; q.taps = nullptr;
    DG_HIP(dg_launch_pre_general(q, c.stream));
    if (int rc = p.plane() ? plane_sample(c, false) : (p.direct() ? direct_sample(c, false) : transpose_maps(c))) return rc;
    DgGatherArgs g;
    memset(&g, 0, sizeof(g));
    g.B = p.B; g.S = p.S; g.Sh = p.Sh; g.P = p.P; g.Ppad = p.Ppad; g.KF = p.KF; g.KD = p.KD;
    int nj = 0;
    for (int o = 0; o < p.nopx(); ++o) {
        // (the intra feature operand: its own feature rows / map, and operand 0's code once more as the C part of its blobs)
        const int srcsel = p.ops[o].srcsel;
        const int64_t* idx = p.sampled_rows() ? nullptr : c.op_map(o);       // (the samplers' rows are sampled through the batch maps already)
        DgGatherJob& f = g.jobs[nj++];
        f.src = p.sampled_rows() ? f32(c.ws, p.rows_f[o]) : f32(c.ws, o == p.xop ? p.nhwc_x : p.nhwc_f[srcsel]); f.coords = c.coords(o); f.srcidx = idx;
        f.blob = c.ws + p.op[o]; f.inv_norm = nullptr; f.colpart = f32(c.ws, p.colpart[o]);
        f.ext_inv = c.feat_inv ? c.feat_inv + (size_t)o * p.B * p.P : nullptr;
        f.K = p.C; f.K4 = p.C4; f.Kpad = p.KF; f.is_code = 0; f.h = p.h; f.w = p.w;
        DgGatherJob& k = g.jobs[nj++];
        k.src = p.sampled_rows() ? f32(c.ws, p.rows_c[o]) : f32(c.ws, p.nhwc_c[srcsel]); k.coords = c.coords(o); k.srcidx = idx;
        k.blob = c.ws + p.op[o]; k.inv_norm = f32(c.ws, p.inv[o]); k.colpart = f32(c.ws, p.ccolpart[o]);
        k.K = p.D; k.K4 = p.D4; k.Kpad = p.KD; k.is_code = 1; k.h = p.hc; k.w = p.wc;
    }
    g.njobs = nj;
    g.direct = p.sampled_rows() ? 1 : 0;
    // exact clamp masks of the small sample grids: the sign of every fp32 code dot product from the sampled rows
    // (k_plane_sample's, like the gather's input) - extra blocks of the gather launch (its own launch until round 4)
    if (p.masks == Masks::Sampled) cd_mask_args(c, p.rows_c, g.cd);
    g.pre = pre_late;
    DG_HIP(dg_launch_gather(g, p.KF, c.stream));
    return DG_OK;
}

// 3. column sums of the operands (mean feats for the centering, code sums for the cd means)
static int fwd_colmeans(Fwd& c) {
    const Plan& p = c.p;
    const DgCorrArgs& a = c.a;
    DgColmeanArgs m;
    memset(&m, 0, sizeof(m));
    m.nops = p.nopx(); m.B = p.B; m.P = p.P; m.Ppad = p.Ppad; m.KF = p.KF; m.KD = p.KD;
    for (int o = 0; o < p.nopx(); ++o) {
        m.colpart[o] = p.pointwise ? f32(c.ws, p.colpart[o]) : nullptr; m.bbar[o] = f32(c.ws, p.bbar[o]);
        m.bsplit[o] = reinterpret_cast<__bf16*>(c.ws + p.bsplit[o]);
        m.ngroups[o] = p.Ppad / 32;              // feats partial column sums: one group per tile on both paths
        m.ccolpart[o] = f32(c.ws, p.ccolpart[o]); m.csum[o] = f32(c.ws, p.csum[o]);
    }
    m.zero_word = p.depth_in_gs() ? reinterpret_cast<unsigned int*>(c.ws + p.ticket) : nullptr;
    m.zero_words9 = a.wctr;
    if (p.gr_on) {             // the consumer lists of k_corr2's grouped ragged blocks ride along (extra blocks of this launch)
        m.gr.nh = p.T; m.gr.nkeys = p.gr_nkeys; m.gr.B = p.B;
        for (int t = 0; t < p.T; ++t) { m.gr.sidx[t] = p.map_of(t, c.perms); m.gr.key[t] = p.gr_key[t]; }
        m.gr.list = reinterpret_cast<int32_t*>(c.ws + p.gr_list); m.gr.count = reinterpret_cast<int32_t*>(c.ws + p.gr_count);
        m.gr.rank = reinterpret_cast<int16_t*>(c.ws + p.gr_rank);
    }
    if (p.dense() && p.pointwise) {       // dense code operands from channel planes (norms: k_prep_dense; csum: k_rowmean launch)
        m.dc.code[0] = c.code; m.dc.code[1] = c.code_pos;
        for (int o = 0; o < 2; ++o) { m.dc.blob[o] = c.ws + p.op[o]; m.dc.inv_norm[o] = f32(c.ws, p.inv[o]); m.dc.ccolpart[o] = f32(c.ws, p.ccolpart[o]); }
        m.dc.B = p.B; m.dc.D = p.D; m.dc.KF = p.KF; m.dc.KD = p.KD; m.dc.h = p.h; m.dc.w = p.w; m.dc.P = p.P; m.dc.Ppad = p.Ppad;
        if (p.masks == Masks::DenseSplit) { m.dc.clo[0] = c.ws + p.clo[0]; m.dc.clo[1] = c.ws + p.clo[1]; }
    }
    if (c.split) {
        DgColmeanArgs ms = m;
        ms.zsel = 1; m.zsel = 2;
        DG_HIP(c.side->hand_over(0));                        // the draw (and the norms): the consumer lists below read the batch maps
        DG_HIP(dg_launch_colmean(ms, c.side->stream()));     // code operands (+ what the fp16 C parts drop)
    }
    DG_HIP(dg_launch_colmean(m, c.stream));
    return DG_OK;
}

// exact clamp masks on the dense grid with `pointwise`: cd from split fp16 operands (the C parts + what they drop, both written by
// fwd_colmeans' launch)
static int fwd_cd_mask3(Fwd& c) {
    const Plan& p = c.p;
    DgCdMask3Args m;
    memset(&m, 0, sizeof(m));
    m.opR = c.ws + p.op[0]; m.loR = c.ws + p.clo[0];
    for (int t = 0; t < p.T; ++t) {
        m.opS[t] = c.ws + p.op[p.ps[t].op]; m.loS[t] = c.ws + p.clo[p.ps[t].op]; m.sidx[t] = p.map_of(t, c.perms);
        m.bits[t] = reinterpret_cast<uint32_t*>(c.ws + p.maskbits[t]);
    }
    m.T = p.T; m.B = p.B; m.Ppad = p.Ppad; m.blob_bytes = p.blob; m.off_c = p.blob_off_c; m.KD = p.KD;
    if (c.split) {
        DG_HIP(c.side->hand_over(1));                        // the code operands: k_rowmean reduces their column sums and writes FOLD's
                                                             // stash into the padding they zeroed
        DG_HIP(dg_launch_cd_mask3(m, c.side->stream()));
        DG_HIP(c.side->record_join());
    } else {
        DG_HIP(dg_launch_cd_mask3(m, c.stream));
    }
    return DG_OK;
}

// the row means of fd (pointwise centering as a rank-1 correction)
static int fwd_rowmeans(Fwd& c) {
    const Plan& p = c.p;
    DgRowmeanArgs r;
    memset(&r, 0, sizeof(r));
    r.B = p.B; r.P = p.P; r.Ppad = p.Ppad; r.KF = p.KF; r.KD = p.KD; r.njobs = p.T; r.abar = f32(c.ws, p.bbar[0]);
    for (int t = 0; t < p.T; ++t) {
        r.jobs[t].A = c.ws + p.op[p.ps[t].rop]; r.jobs[t].aidx = nullptr;
        r.jobs[t].bbar = f32(c.ws, p.bbar[p.ps[t].op]); r.jobs[t].bidx = p.map_of(t, c.perms);
        r.jobs[t].bsplit = reinterpret_cast<const __bf16*>(c.ws + p.bsplit[p.ps[t].op]);
        r.jobs[t].rvec = f32(c.ws, p.rvec[t]); r.jobs[t].rimg = f32(c.ws, p.rimg[t]);
    }
    if (p.dense()) {
        r.ncs = 2;
        for (int o = 0; o < 2; ++o) { r.cs_part[o] = f32(c.ws, p.ccolpart[o]); r.cs_out[o] = f32(c.ws, p.csum[o]); }
    }
    if (p.xop >= 0) {         // job 0's stationary operand is its own: k_rowmean<true> (the kernel reads ONE set of blobs for all other jobs)
        r.xA = c.ws + p.op[p.xop]; r.xabar = f32(c.ws, p.bbar[p.xop]);
        r.jobs[0].A = c.ws + p.op[0];
    }
    if (p.fold) { r.stash = c.ws + p.op[p.ps[0].rop]; r.stash_off = FOLD_STASH_OFF; }
    DG_HIP(dg_launch_rowmean(r, c.stream));
    return DG_OK;
}

// 5. scalar outputs: the partial sums are reduced by the next launch (k_gs on a gradient pass)
static int fwd_finish(Fwd& c) {
    const Plan& p = c.p;
    const DgCorrArgs& a = c.a;
    DgFinishArgs f;
    memset(&f, 0, sizeof(f));
    for (int j = 0; j < a.njobs; ++j) {
        f.part[j] = a.jobs[j].part; f.slot_loss[j] = a.jobs[j].slot_loss; f.slot_cd[j] = a.jobs[j].slot_cd;
        f.scale[j] = a.jobs[j].fin_scale;
    }
    f.njobs = a.njobs; f.nblk = p.B * p.nrb; f.B = p.B; f.P = p.P;
    if (p.depth_in_gs()) {                                     // the depth blocks' partial sums: one more entry of the reduction
        const int j = f.njobs++;
        f.part[j] = f32(c.ws, p.part[p.T]); f.slot_loss[j] = DG_OUT_LOSS_DEPTH; f.slot_cd[j] = -1;
        f.scale[j] = p.inv_numel;
        f.nblk_job[j] = p.B * p.dep_nrb;
    }
    f.nzsum = p.depth ? f32(c.ws, p.nzsum) : nullptr;
    f.out = c.out;
    f.wtot[0] = c.desc->w_intra; f.wtot[1] = c.desc->w_inter; f.wtot[2] = c.desc->w_neg; f.wtot[3] = c.desc->w_depth;
    if (!p.grad) {
        DG_HIP(dg_launch_finish(f, c.stream));
        return DG_OK;
    }
    DgGsArgs g;
    const uint32_t* dep_maskbits = nullptr;
    build_gs_jobs(p, c.ws, c.perms, g);
    g.fin = f;
    if (p.depth) {
        g.dep_op = c.ws + p.op[0]; g.dep_nz = f32(c.ws, p.nz); g.dep_dR = f32(c.ws, p.dRA[p.T]); g.dep_part = f32(c.ws, p.part[p.T]);
        g.dep_ticket = reinterpret_cast<unsigned int*>(c.ws + p.ticket);
        dep_maskbits = p.has_masks() ? reinterpret_cast<const uint32_t*>(c.ws + p.maskbits[0]) : nullptr;   // cd of the depth term = intra's cd
        g.dep_shift = p.shift_depth; g.dep_nrb = p.dep_nrb; g.dep_blocks = p.B * p.dep_nrb;
        g.dep_lo = p.lo; g.dep_hi = p.hi;
    }
    if (p.depth_run != Depth::GsOwnLaunch) {
        DG_HIP(dg_launch_gs(g, dep_maskbits, c.stream, false, p.half));
        return DG_OK;
    }
    // the G-stream blocks as a launch of the plain kernel (two blocks per CU) and the depth blocks alone in the masked form
    // (256 registers per wave; the last depth block reduces the call's partial sums) - SIDE BY SIDE on a second stream
    // where the library has one (fork / join by events, capturable into a hipGraph): the stream launch is bound by HBM
    // bytes, the 128 depth blocks by a latency chain on half the CUs (one behind the other: 76 + 52 us)
    DgGsArgs gstream = g;
    gstream.dep_blocks = 0; gstream.fin.out = nullptr;
    if (!c.side) c.side.emplace(c.stream);
    SideRegion& side = *c.side;
    side.reset();                                     // (a second fork .. join of the same region object)
    if (side) {
        DG_HIP(side.fork());
        DG_HIP(dg_launch_gs(g, dep_maskbits, side.stream(), true));
        DG_HIP(side.record_join());
        DG_HIP(dg_launch_gs(gstream, nullptr, c.stream, false, p.half));
        DG_HIP(side.join());
    } else {
        DG_HIP(dg_launch_gs(gstream, nullptr, c.stream, false, p.half));
        DG_HIP(dg_launch_gs(g, dep_maskbits, c.stream, true));
    }
    return DG_OK;
}

static int corr_forward_impl(const dg_corr_desc* desc, const FwdInputs& in, float* out_scalars, void* workspace, size_t workspace_bytes,
                             dg_stream_t stream_) {
    Fwd c(in);
    if (int rc = make_plan(desc, c.p, in.intra_entry)) return rc;
    const Plan& p = c.p;
    c.desc = desc; c.out = out_scalars; c.stream = static_cast<hipStream_t>(stream_);
    if (int rc = fwd_validate(c, workspace, workspace_bytes)) return rc;

    // Exact clamp masks on the dense grid (round 6): the mask words depend on the code maps and the batch maps only, so their chain
    // (code norms + draw -> code operands -> k_cd_mask3) runs on the library's side stream BESIDE the feature side of the preparation
    // (k_prep_dense's feats, k_colmean, k_rowmean) instead of in front of the fused kernel: the same launches split by role, joined
    // in front of the fused kernel.  Without a side stream (first call inside a capture) everything runs in sequence as before.
    if (p.dense_masks() && split_masks_enabled()) c.side.emplace(c.stream);
    c.split = c.side && static_cast<bool>(*c.side) && p.pointwise;

    // 1.+2. operands
    if (p.small()) return forward_small(c);         // (sampled coordinates on a small grid: one fused kernel)
    if (int rc = p.dense() ? fwd_operands_dense(c) : fwd_operands_general(c)) return rc;

    // (the job table of step 4 is needed here already: the consumer lists of k_corr2's grouped ragged blocks are written by
    //  extra blocks of the k_colmean launch)
    build_corr_jobs(p, c.ws, c.perms, c.a);

    // 3. column sums of the operands, the exact masks that need them, then the row means of fd
    if (int rc = fwd_colmeans(c)) return rc;
    if (p.masks == Masks::DenseSplit) { if (int rc = fwd_cd_mask3(c)) return rc; }
    if (p.pointwise) { if (int rc = fwd_rowmeans(c)) return rc; }

    // 4. fused correlation passes
    if (c.split) DG_HIP(c.side->join());                        // the mask words
    if (int rc = launch_main(p, c.a, c.stream)) return rc;

    // 5. scalar outputs
    return fwd_finish(c);
}

extern "C" int dg_corr_forward(const dg_corr_desc* desc, const float* orig_feats, const float* orig_feats_pos,
                               const float* orig_code, const float* orig_code_pos, const float* depth,
                               const float* coords1, const float* coords2, const int64_t* perms,
                               float* out_scalars, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    const FwdInputs in{orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms};
    return corr_forward_impl(desc, in, out_scalars, workspace, workspace_bytes, stream_);
}

extern "C" int dg_corr_forward_extnorm(const dg_corr_desc* desc, const float* orig_feats, const float* orig_feats_pos,
                                       const float* orig_code, const float* orig_code_pos, const float* depth,
                                       const float* coords1, const float* coords2, const int64_t* perms, const float* feat_inv,
                                       float* out_scalars, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!feat_inv) return fail(DG_ERR_INVALID, "dg_corr_forward_extnorm: feat_inv is null");
    if (desc && desc->h > 0 && desc->w > 0 && (size_t)desc->h * desc->w > DG_CHANNEL_LAST_MAX_POS)
        return fail(DG_ERR_UNSUPPORTED, "dg_corr_forward_extnorm: feature map %dx%d too large (max %d positions)", desc->h, desc->w, DG_CHANNEL_LAST_MAX_POS);
    FwdInputs in{orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms};
    in.feat_inv = feat_inv;
    return corr_forward_impl(desc, in, out_scalars, workspace, workspace_bytes, stream_);
}

extern "C" int dg_sampled_sumsq(int32_t B, int32_t C, int32_t h, int32_t w, int32_t S, int32_t line_grid, const float* feats,
                                const float* coords, const int64_t* srcidx, int32_t accumulate, float* out, dg_stream_t stream_) {
    if (B < 1 || C < 1 || h < 1 || w < 1 || S < 1 || !feats || !coords || !out) return fail(DG_ERR_INVALID, "dg_sampled_sumsq: bad arguments");
    if ((size_t)h * w > DG_CHANNEL_LAST_MAX_POS)
        return fail(DG_ERR_UNSUPPORTED, "dg_sampled_sumsq: feature map %dx%d too large (max %d positions)", h, w, DG_CHANNEL_LAST_MAX_POS);
    DG_HIP(dg_launch_sampled_sumsq(feats, coords, srcidx, out, B, C, h, w, S, line_grid ? 1 : S, accumulate ? 1 : 0, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_sample_rows(const float* map, const float* coords, const int64_t* srcidx, int32_t B, int32_t K, int32_t h, int32_t w,
                              int32_t S, int32_t Sh, int32_t Kout, int32_t as_bf16, void* out, dg_stream_t stream_) {
    if (!map || !coords || !out) return fail(DG_ERR_INVALID, "dg_sample_rows: null pointer");
    if (((uintptr_t)map | (uintptr_t)coords | (uintptr_t)out) & 3) return fail(DG_ERR_INVALID, "dg_sample_rows: map, coords and out must be 4-byte aligned");
    if ((uintptr_t)srcidx & 7) return fail(DG_ERR_INVALID, "dg_sample_rows: srcidx must be 8-byte aligned");
    if (B < 1 || K < 1 || h < 1 || w < 1 || S < 1 || Sh < 1)
        return fail(DG_ERR_INVALID, "dg_sample_rows: non-positive dimension (B=%d K=%d map %dx%d grid %dx%d)", B, K, h, w, Sh, S);
    if ((size_t)h * w > DG_SAMPLE_DIRECT_MAX_POS)
        return fail(DG_ERR_UNSUPPORTED, "dg_sample_rows: map %dx%d too large (max %d positions)", h, w, DG_SAMPLE_DIRECT_MAX_POS);
    if (Kout < K || Kout % 4 != 0) return fail(DG_ERR_INVALID, "dg_sample_rows: Kout=%d must be a multiple of 4 and at least K=%d", Kout, K);
    if (B > 65535 || (int64_t)S * Sh > (1 << 24)) return fail(DG_ERR_UNSUPPORTED, "dg_sample_rows: B=%d (max 65535) or a grid of %dx%d (max 2^24 positions)", B, Sh, S);
    DgSampleDirectArgs g;
    memset(&g, 0, sizeof(g));
    g.src[0] = map; g.coords[0] = coords; g.srcidx[0] = srcidx; g.rows[0] = out;
    g.K[0] = K; g.Kout[0] = Kout; g.as_bf16[0] = as_bf16 ? 1 : 0; g.h[0] = h; g.w[0] = w;
    g.njobs = 1; g.B = B; g.S = S; g.Sh = Sh; g.P = S * Sh;
    DG_HIP(dg_launch_sample_direct(g, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_corr_forward_draw(const dg_corr_desc* desc, const float* orig_feats, const float* orig_feats_pos,
                                    const float* orig_code, const float* orig_code_pos, const float* depth,
                                    const float* coords1, const float* coords2, int64_t* perms_out, uint64_t seed, void* perm_state,
                                    float* out_scalars, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!desc) return fail(DG_ERR_INVALID, "null descriptor");
    if (desc->n_neg > 0 && !perms_out) return fail(DG_ERR_INVALID, "perms_out is null with n_neg=%d", desc->n_neg);
    const DrawArgs draw{perms_out, seed, static_cast<unsigned long long*>(perm_state)};
    FwdInputs in{orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms_out};
    in.draw = &draw;
    return corr_forward_impl(desc, in, out_scalars, workspace, workspace_bytes, stream_);
}

extern "C" int dg_corr_forward_intra_feats(const dg_corr_desc* desc, const float* orig_feats, const float* orig_feats_pos,
                                           const float* orig_code, const float* orig_code_pos, const float* depth,
                                           const float* coords1, const float* coords2, int64_t* perms, int32_t draw_perms, uint64_t seed,
                                           void* perm_state, const float* intra_feats,
                                           float* out_scalars, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!desc) return fail(DG_ERR_INVALID, "null descriptor");
    if (desc->n_neg > 0 && !perms) return fail(DG_ERR_INVALID, "perms is null with n_neg=%d", desc->n_neg);
    const DrawArgs draw{perms, seed, static_cast<unsigned long long*>(perm_state)};
    FwdInputs in{orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms};
    in.draw = draw_perms ? &draw : nullptr; in.intra = intra_feats; in.intra_entry = true;
    return corr_forward_impl(desc, in, out_scalars, workspace, workspace_bytes, stream_);
}

extern "C" int dg_corr_forward_masked(const dg_corr_desc* desc, const float* orig_feats, const float* orig_feats_pos,
                                      const float* orig_code, const float* orig_code_pos, const float* depth,
                                      const float* coords1, const float* coords2, int64_t* perms, int32_t draw_perms, uint64_t seed,
                                      void* perm_state, const float* feat_keep, const float* feat_pos_keep, float keep_scale,
                                      float* out_scalars, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!desc) return fail(DG_ERR_INVALID, "null descriptor");
    if (desc->n_neg > 0 && !perms) return fail(DG_ERR_INVALID, "perms is null with n_neg=%d", desc->n_neg);
    if ((feat_keep || feat_pos_keep) && !(keep_scale > 0.f)) return fail(DG_ERR_INVALID, "keep_scale %g with keep flags", (double)keep_scale);
    const DrawArgs draw{perms, seed, static_cast<unsigned long long*>(perm_state)};
    const FeatKeep fk{{feat_keep, feat_pos_keep}, keep_scale};
    FwdInputs in{orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms};
    in.draw = draw_perms ? &draw : nullptr; in.fk = &fk;
    return corr_forward_impl(desc, in, out_scalars, workspace, workspace_bytes, stream_);
}

// ---- the backward: the source table of the one k_scatter launch, filled from the pair-set table
struct ScatterFill {
    DgScatterArgs& s;
    char* ws;
    void add(size_t buf, const int64_t* route, int gidx, int csel, float factor, int dest, int raw, int half = 0, const float* dfac = nullptr) {
        DgScatterSrc& q = s.src[s.nsrc++];
        q.buf = f32(ws, buf); q.route = route; q.gidx = gidx; q.coords_sel = csel;
        q.factor = factor; q.dest = dest; q.raw = raw; q.half = half; q.dfac = dfac;
    }
};

// the fused small-grid kernel (dg_small.hip): stationary-side tiles raw, streamed-side tiles final (one set per half of the
// stationary tiles), and with `pointwise` the same again for the old_mean term, whose factor old_mean_t lives on the device
static void scatter_sources_small(const Plan& p, const int64_t* perms, ScatterFill& f) {
    DgScatterArgs& s = f.s;
    char* ws = f.ws;
    for (int t = 0; t < p.T; ++t) {
        const PairSet& q = p.ps[t];
        const int64_t* route = p.batch_map(q.neg, perms);
        const float* om = p.pointwise ? f32(ws, p.om) + t : nullptr;
        f.add(p.dRA[t], nullptr, q.gidx, 0, q.factor, 0, 1);
        if (p.pointwise) f.add(p.dRA2[t], nullptr, q.gidx, 0, q.factor, 0, 1, 0, om);
        // the streamed-side (final) tiles: one set per half of the stationary tiles, with `pointwise` the old_mean terms on top.
        // ROUTED sources (the negatives) are merged into one buffer each by extra slices of the combine launch, in front of the
        // adjoint launch that reads the result - routed sources are what that launch's time scales with.  Direct ones (intra,
        // inter) are read by the combine launch itself: those keep their terms.
        if (route && (p.pointwise || p.nsplit == 2)) {
            const int j = s.naxpy++;
            s.axo[j] = f32(ws, p.dRBm[t]); s.axd[j] = f32(ws, p.dRB[t]); s.axd2[j] = p.nsplit == 2 ? f32(ws, p.dRBs[t]) : nullptr;
            s.axs[j] = p.pointwise ? f32(ws, p.dRB2[t][0]) : nullptr; s.axs2[j] = (p.pointwise && p.nsplit == 2) ? f32(ws, p.dRB2[t][1]) : nullptr;
            s.axf[j] = om;
            f.add(p.dRBm[t], route, q.gidx, q.csel, q.factor, q.dest, 0);
        } else {
            for (int k = 0; k < p.nsplit; ++k) {
                f.add(k == 0 ? p.dRB[t] : p.dRBs[t], route, q.gidx, q.csel, q.factor, q.dest, 0);
                if (p.pointwise) f.add(p.dRB2[t][k], route, q.gidx, q.csel, q.factor, q.dest, 0, 0, om);
            }
        }
    }
}

// the blob kernels.  dRA[t]: the fused kernel's raw accumulator-order tiles (stationary operand = operand 1 for every pair-set);
// dRB[t]: k_gs output, row-major, normalisation backward already applied.  Where the intra pair-set's -G is symmetric
// (Plan::intra_symmetric: no k_gs job, build_gs_jobs) d/dc1 + d/dc2 = 2 d/dc1
static void scatter_sources_blobs(const Plan& p, const int64_t* perms, ScatterFill& f) {
    const int hf = p.half ? 1 : 0;              // (the pair-sets' tiles of k_corr2 and k_gs; the depth term's stay fp32)
    for (int t = 0; t < p.T; ++t) {
        const PairSet& q = p.ps[t];
        const bool doubled = t == 0 && p.intra_symmetric();
        f.add(p.dRA[t], nullptr, q.gidx, 0, doubled ? 2.0f * q.factor : q.factor, 0, 1, hf);
        if (!doubled) f.add(p.dRB[t], p.batch_map(q.neg, perms), q.gidx, q.csel, q.factor, q.dest, 0, hf);
    }
}

static int corr_backward_impl(const dg_corr_desc* desc, const float* grad_scalars, const float* grad_total, const float* coords1,
                              const float* coords2, const int64_t* perms, float* grad_code, float* grad_code_pos,
                              void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    Plan p{};
    int rc = make_plan(desc, p);
    if (rc != DG_OK) return rc;
    if (!p.grad) return fail(DG_ERR_INVALID, "dg_corr_backward needs a descriptor with DG_NEED_GRAD (as used in forward)");
    if (!coords1 || !coords2 || !grad_code || !grad_code_pos || !workspace) return fail(DG_ERR_INVALID, "null pointer");
    if (p.N > 0 && !perms) return fail(DG_ERR_INVALID, "perms is null with n_neg=%d", p.N);
    if (workspace_bytes < p.total) return fail(DG_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, p.total);
    char* ws = static_cast<char*>(workspace);
    DgScatterArgs s;
    memset(&s, 0, sizeof(s));
    ScatterFill fill{s, ws};
    if (p.small()) scatter_sources_small(p, perms, fill);
    else scatter_sources_blobs(p, perms, fill);
    if (p.depth) fill.add(p.dRA[p.T], nullptr, 3, 0, 2.0f * p.grad_f, 0, 1);   // dd and cd symmetric: d/dc1 + d/dc2 = 2 d/dc1
    s.coords1 = coords1; s.coords2 = coords2; s.gscal = grad_scalars; s.gtot = grad_total;
    s.wtot[0] = desc->w_intra; s.wtot[1] = desc->w_inter; s.wtot[2] = desc->w_neg; s.wtot[3] = desc->w_depth;
    s.comb[0] = f32(ws, p.comb[0]); s.comb[1] = f32(ws, p.comb[1]);
    s.taps = ws + p.taps;
    s.xop = ws + p.op[0]; s.xinv = f32(ws, p.inv[0]); s.blob_bytes = p.blob; s.blob_off_c = p.blob_off_c;
    // (half, final sources: destination 0 = the code map behind operand 0 - the negatives' streamed operand on the shared grid -,
    //  destination 1 = operand 1's)
    s.xinv_dest[0] = f32(ws, p.inv[0]); s.xinv_dest[1] = p.nops > 1 ? f32(ws, p.inv[1]) : nullptr;
    s.out[0] = grad_code; s.out[1] = grad_code_pos;
    s.B = p.B; s.D = p.D; s.DP = p.KD; s.h = p.hc; s.w = p.wc; s.S = p.S; s.Sh = p.Sh; s.P = p.P; s.Ppad = p.Ppad;     // (h, w): the code maps
    if ((size_t)p.hc * p.wc > 4096) return fail(DG_ERR_UNSUPPORTED, "code map %dx%d too large for the gradient gather (max 4096 pixels)", p.hc, p.wc);
    s.DC = 8;
    s.dense = p.dense() ? 1 : 0;
    s.taps_ready = p.dense() ? 0 : 1;          // (general coordinates: built by the forward's first launch, dg_launch_pre_general)
    DG_HIP(dg_launch_scatter(s, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_corr_backward(const dg_corr_desc* desc, const float* grad_scalars, const float* coords1,
                                const float* coords2, const int64_t* perms, float* grad_code, float* grad_code_pos,
                                void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!grad_scalars) return fail(DG_ERR_INVALID, "null pointer");
    return corr_backward_impl(desc, grad_scalars, nullptr, coords1, coords2, perms, grad_code, grad_code_pos, workspace,
                              workspace_bytes, stream_);
}

extern "C" int dg_corr_backward_total(const dg_corr_desc* desc, const float* grad_total, const float* coords1,
                                      const float* coords2, const int64_t* perms, float* grad_code, float* grad_code_pos,
                                      void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (!grad_total) return fail(DG_ERR_INVALID, "null pointer");
    return corr_backward_impl(desc, nullptr, grad_total, coords1, coords2, perms, grad_code, grad_code_pos, workspace,
                              workspace_bytes, stream_);
}

static int materialize_impl(const dg_corr_desc* desc, int32_t which, const int64_t* perms, float* out_cd, float* out_loss,
                            void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    Plan p{};
    int rc = make_plan(desc, p);
    if (rc != DG_OK) return rc;
    if (!workspace) return fail(DG_ERR_INVALID, "null workspace");
    if (workspace_bytes < p.total) return fail(DG_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, p.total);
    if (which < -1 || which >= p.T) return fail(DG_ERR_INVALID, "which=%d outside [-1,%d)", which, p.T);
    if (which == -1 && !p.depth) return fail(DG_ERR_INVALID, "depth term not enabled in descriptor");
    if (which >= 2 && p.shared && !perms)
        return fail(DG_ERR_INVALID, "materialising a negative of a DG_SHARED_COORDS call needs its batch maps: dg_corr_materialize_shared");
    if (!out_cd && !out_loss) return DG_OK;
    char* ws = static_cast<char*>(workspace);
    if (p.small()) {        // the fused small-grid kernel again, on the rows (and old_mean_t) the forward left in the workspace
        DgSmallArgs m;
        small_args(p, desc, ws, perms, m);
        m.mat = 1; m.mat_t = which; m.out_cd = out_cd; m.out_loss = out_loss; m.grad = 0; m.span = nullptr;
        DG_HIP(dg_launch_corr_small(m, static_cast<hipStream_t>(stream_)));
        return DG_OK;
    }
    // (a gradient pass with k_corr2's FOLD left the intra row means in the padding of the operand-1 blobs' C part: k_corr_main's
    //  un-reduced forms multiply all of it.  Cleared for this launch and written back behind it, from the row means that are still in
    //  the workspace: the workspace stays what the forward prepared - dg_corr_relaunch_main remains valid.)
    const int stash_off = p.blob_off_c + FOLD_STASH_OFF;
    if (p.fold)
        DG_HIP(dg_launch_set_stash(ws + p.op[0], p.B, p.Ppad / 32, (size_t)p.blob, stash_off, nullptr, p.P, p.Ppad, static_cast<hipStream_t>(stream_)));
    DgCorrArgs a;
    corr_args_base(p, ws, a);
    // stationary = operand 2 (on MFMA lanes) -> the stores of one accumulator register are contiguous along q
    DgJob j = which == -1 ? depth_job(p, ws) : helper_job(p, ws, which, true, perms);
    j.center_on_lane = 0;
    j.out_cd = out_cd; j.out_loss = out_loss; j.part = nullptr; j.dR = nullptr;
    a.jobs[0] = j; a.njobs = 1;
    a.pos_w = p.dense() ? p.w : 0;
    DG_HIP(dg_launch_corr(a, p.KF, p.KD, p.rf, 2, static_cast<hipStream_t>(stream_)));
    if (p.fold)
        DG_HIP(dg_launch_set_stash(ws + p.op[0], p.B, p.Ppad / 32, (size_t)p.blob, stash_off, reinterpret_cast<const float*>(ws + p.rvec[0]),
                                   p.P, p.Ppad, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_corr_materialize(const dg_corr_desc* desc, int32_t which, float* out_cd, float* out_loss,
                                   void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    return materialize_impl(desc, which, nullptr, out_cd, out_loss, workspace, workspace_bytes, stream_);
}

extern "C" int dg_corr_materialize_shared(const dg_corr_desc* desc, int32_t which, const int64_t* perms, float* out_cd, float* out_loss,
                                          void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    return materialize_impl(desc, which, perms, out_cd, out_loss, workspace, workspace_bytes, stream_);
}

// Histograms of the pair-sets' cd from the operands the forward left in the workspace (dg_hist.hip): one memset node and one launch,
// the pair-set as a grid dimension.  Reads the workspace only - a later dg_corr_backward sees what the forward wrote.
extern "C" int dg_corr_cd_hist(const dg_corr_desc* desc, int32_t first, int32_t count, const int64_t* perms, int32_t nbins, float lo,
                               float hi, int64_t* out_counts, void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    Plan p{};
    int rc = make_plan(desc, p);
    if (rc != DG_OK) return rc;
    if (first < 0)
        return fail(DG_ERR_INVALID, "dg_corr_cd_hist: first=%d: pair-sets start at 0 (the depth term's element is dd, which has no cd histogram)", first);
    if (count < 1 || first > p.T - count) return fail(DG_ERR_INVALID, "dg_corr_cd_hist: pair-sets [%d,%d) outside [0,%d)", first, first + count, p.T);
    if (nbins < 1 || nbins > DG_HIST_MAX_BINS) return fail(DG_ERR_INVALID, "dg_corr_cd_hist: nbins=%d outside [1,%d]", nbins, DG_HIST_MAX_BINS);
    if (!__builtin_isfinite(lo) || !__builtin_isfinite(hi) || !(lo < hi))
        return fail(DG_ERR_INVALID, "dg_corr_cd_hist: the range needs finite lo < hi, got [%g,%g]", (double)lo, (double)hi);
    if (!out_counts || !workspace) return fail(DG_ERR_INVALID, "null pointer");
    if (workspace_bytes < p.total) return fail(DG_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, p.total);
    if (first + count > 2 && p.shared && !perms)
        return fail(DG_ERR_INVALID, "dg_corr_cd_hist: a negative of a DG_SHARED_COORDS call needs its batch maps (perms)");
    char* ws = static_cast<char*>(workspace);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DgCdHistArgs a;
    memset(&a, 0, sizeof(a));
    a.opR = ws + p.op[0]; a.rowsR = f32(ws, p.rows_c[0]);
    for (int j = 0; j < count; ++j) {
        const int t = first + j, o2 = p.ps[t].op;
        a.opS[j] = ws + p.op[o2]; a.rowsS[j] = f32(ws, p.rows_c[o2]); a.sidx[j] = p.map_of(t, perms);
    }
    a.out = reinterpret_cast<unsigned long long*>(out_counts);
    a.count = count; a.B = p.B; a.P = p.P; a.Ppad = p.Ppad; a.D = p.D; a.D4 = p.D4; a.KD = p.KD;
    a.blob_bytes = p.blob; a.off_c = p.blob_off_c;
    a.nbins = nbins; a.lo = lo; a.scale = (float)nbins / (hi - lo);
    DG_HIP(hipMemsetAsync(out_counts, 0, (size_t)count * nbins * sizeof(int64_t), stream));
    DG_HIP(dg_launch_cd_hist(a, p.hist == Hist::Rows, stream));
    return DG_OK;
}

// Measurement aid: re-launch ONLY the fused correlation kernel on the operands a previous dg_corr_forward
// (same desc / perms / workspace) left in the workspace.  Idempotent (rewrites the same outputs).
extern "C" int dg_corr_relaunch_main(const dg_corr_desc* desc, const int64_t* perms, void* workspace,
                                     size_t workspace_bytes, dg_stream_t stream_) {
    Plan p{};
    int rc = make_plan(desc, p);
    if (rc != DG_OK) return rc;
    if (!workspace || workspace_bytes < p.total) return fail(DG_ERR_WORKSPACE, "workspace missing or too small");
    if (p.N > 0 && !perms) return fail(DG_ERR_INVALID, "perms is null");
    char* ws = static_cast<char*>(workspace);
    if (p.small()) {
        // (the scalars of the re-launch go to the workspace's scratch vector: the call's own outputs are not touched)
        DgSmallArgs m;
        small_args(p, desc, ws, perms, m);
        m.out = f32(ws, p.scratch_out);
        DG_HIP(dg_launch_corr_small(m, static_cast<hipStream_t>(stream_)));        // (the kernel alone: what the roofline leg times)
        return DG_OK;
    }
    DgCorrArgs a;
    build_corr_jobs(p, ws, perms, a);
    return launch_main(p, a, static_cast<hipStream_t>(stream_));
}

extern "C" int dg_corr_intra_folded(const dg_corr_desc* desc) {
    Plan p{};
    if (make_plan(desc, p) != DG_OK) return -1;
    return p.fold ? 1 : 0;
}

extern "C" const char* dg_corr_main_kernel_name(const dg_corr_desc* desc) {
    Plan p{};
    if (make_plan(desc, p) != DG_OK) return nullptr;
    return p.main == MainKernel::Small ? "k_corr_small" : (p.main == MainKernel::Corr2 ? "k_corr2" : "k_corr_main");
}

extern "C" int dg_normalize_split(int32_t B, int32_t C, int32_t h, int32_t w, const float* src, int32_t nchunks, int32_t chunk_c,
                                  float* const* dst, dg_stream_t stream_) {
    if (B < 1 || C < 1 || h < 1 || w < 1 || !src || !dst) return fail(DG_ERR_INVALID, "dg_normalize_split: bad arguments");
    if (nchunks < 1 || nchunks > 16 || chunk_c < 1 || (long long)chunk_c * (nchunks - 1) >= C || (long long)chunk_c * nchunks < C)
        return fail(DG_ERR_INVALID, "dg_normalize_split: %d chunks of %d channels do not tile C=%d (at most 16 chunks)", nchunks, chunk_c, C);
    for (int k = 0; k < nchunks; ++k) if (!dst[k]) return fail(DG_ERR_INVALID, "dg_normalize_split: null destination %d", k);
    DG_HIP(dg_launch_normalize_split(src, B, C, h * w, nchunks, chunk_c, dst, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}
