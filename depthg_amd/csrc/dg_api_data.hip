// C ABI of the gfx950 DepthG library (include/depthg_corr.h), the training data path: the GPU batch augmentation, the batch preparation,
// the frozen-backbone feature cache, the device-resident sample cache, the batch draw of a cached step.
// Host-side only: argument checks and kernel launches on the caller's stream.
#include "dg_api.h"
#include "dg_data_args.h"

#include <vector>

// ---- what the entries share
// the normalisation constants of `who` into mean[3] / stdv[3] (null: 0 / 1): finite, std positive
static int norm_check(const char* who, const float* mean_in, const float* stdv_in, float* mean, float* stdv) {
    for (int c = 0; c < 3; ++c) {
        mean[c] = mean_in ? mean_in[c] : 0.f;
        stdv[c] = stdv_in ? stdv_in[c] : 1.f;
        if (!(stdv[c] > 0.f) || std::isinf(stdv[c]) || !(mean[c] == mean[c]) || std::isinf(mean[c]))
            return fail(DG_ERR_INVALID, "%s: channel %d: mean=%g std=%g", who, c, (double)mean[c], (double)stdv[c]);
    }
    return DG_OK;
}

struct PackedSource {                        // the loader's input as dg_batch_prep and dg_samplecache_put take it
    const uint8_t* packed;
    size_t packed_bytes;
    const int32_t *records_host, *tables_host;
    const void* params;
    int32_t n_records, H, W;
};

// a record that reads a source plane: the plane lies inside `packed` and holds every pixel its sample's tables (xs[W], ys[H]) address
static int batch_source_check(const char* who, int i, const int32_t* r, const int32_t* xs, const PackedSource& P) {
    const int kind = r[0], sw = r[4], sh = r[5];
    const unsigned long long off = (unsigned long long)(uint32_t)r[2] | ((unsigned long long)(uint32_t)r[3] << 32);
    if (sw < 1 || sh < 1) return fail(DG_ERR_INVALID, "%s: record %d: zero-sized source plane %dx%d", who, i, sw, sh);
    if (sw > DG_BATCH_MAX_SIDE || sh > DG_BATCH_MAX_SIDE)
        return fail(DG_ERR_UNSUPPORTED, "%s: record %d: source plane %dx%d above %d a side", who, i, sw, sh, DG_BATCH_MAX_SIDE);
    const unsigned long long bytes = (unsigned long long)sw * sh * (kind == DG_BATCH_IMAGE ? 3 : 1);
    if (!P.packed || off > P.packed_bytes || bytes > P.packed_bytes - off)
        return fail(DG_ERR_INVALID, "%s: record %d: plane of %llu bytes at offset %llu leaves the packed buffer of %zu bytes", who, i, bytes, off,
                    P.packed_bytes);
    const int32_t* ys = xs + P.W;
    for (int x = 0; x < P.W; ++x)
        if (xs[x] < 0 || xs[x] >= sw)
            return fail(DG_ERR_INVALID, "%s: record %d: column table entry %d = %d outside the source width %d (the plane is narrower than the tables address)", who, i, x, xs[x], sw);
    for (int y = 0; y < P.H; ++y)
        if (ys[y] < 0 || ys[y] >= sh)
            return fail(DG_ERR_INVALID, "%s: record %d: row table entry %d = %d outside the source height %d (the plane is shorter than the tables address)", who, i, y, ys[y], sh);
    return DG_OK;
}

// The walk over the host copy of the records of N samples: kind and sample in range, then the caller's own refusals -
// rule(i, r, kind, n, out, twice), with out the record's output (0 image, 1 label, 2 depth) and `twice` set when that output of sample n
// has a record already - then the source plane of a record that reads one.  n_out[o]: the records of output o.
template <class Rule>
static int walk_records(const char* who, const PackedSource& P, int N, int n_out[3], Rule rule) {
    std::vector<uint8_t> seen((size_t)3 * N, 0);
    n_out[0] = n_out[1] = n_out[2] = 0;
    for (int i = 0; i < P.n_records; ++i) {
        const int32_t* r = P.records_host + (size_t)i * DG_BATCH_REC_WORDS;
        const int kind = r[0], n = r[1];
        if (kind < DG_BATCH_IMAGE || kind > DG_BATCH_LABEL_FILL) return fail(DG_ERR_INVALID, "%s: record %d: unknown kind %d (0 .. 4)", who, i, kind);
        if (n < 0 || n >= N) return fail(DG_ERR_INVALID, "%s: record %d: sample %d outside 0 .. %d", who, i, n, N - 1);
        const int out = kind == DG_BATCH_IMAGE ? 0 : (kind == DG_BATCH_LABEL || kind == DG_BATCH_LABEL_FILL) ? 1 : 2;
        if (int rc = rule(i, r, kind, n, out, seen[(size_t)out * N + n]++ != 0)) return rc;
        ++n_out[out];
        if (kind == DG_BATCH_DEPTH_PLANE || kind == DG_BATCH_LABEL_FILL) continue;      // no source
        if (int rc = batch_source_check(who, i, r, P.tables_host + (size_t)n * (P.W + P.H), P)) return rc;
    }
    return DG_OK;
}

static DgLoaderSource loader_source(const PackedSource& P) {
    DgLoaderSource S;
    S.packed = P.packed;
    S.recs = static_cast<const int32_t*>(P.params);
    S.tables = S.recs + (size_t)P.n_records * DG_BATCH_REC_WORDS;
    S.n_records = P.n_records; S.H = P.H; S.W = P.W;
    S.tiles_x = (P.W + DG_BATCH_TW - 1) / DG_BATCH_TW; S.tiles_y = (P.H + DG_BATCH_TH - 1) / DG_BATCH_TH;
    return S;
}

static DgCachePlanes cache_planes(int64_t n_images, int32_t has_labels, int32_t with_depth) {
    return {n_images, 3 + has_labels + with_depth, has_labels ? 3 : -1, with_depth ? 3 + has_labels : -1};
}

// ---- GPU batch augmentation (dg_augment.hip)
static bool augment_sizes_ok(int32_t B, int32_t h, int32_t w) { return B >= 1 && B <= 65535 && h >= 3 && w >= 3 && h <= 16384 && w <= 16384; }

static int augment_stat_blocks(int32_t h, int32_t w) {
    const long long tiles = (long long)((h + DG_AUGM_TH - 1) / DG_AUGM_TH) * ((w + DG_AUGM_TW - 1) / DG_AUGM_TW);
    return (int)(tiles < DG_AUGM_STAT_BLOCKS ? tiles : DG_AUGM_STAT_BLOCKS);
}

extern "C" size_t dg_augment_workspace_bytes(int32_t B, int32_t h, int32_t w) {
    if (!augment_sizes_ok(B, h, w)) return 0;
    return up((size_t)B * augment_stat_blocks(h, w) * sizeof(double), 256);
}

extern "C" int dg_augment_forward(const float* img, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w,
                                  const int32_t* records_host, const void* params, const float* mean, const float* stdv, int32_t B,
                                  int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, float* img_aug, float* coord_aug,
                                  void* workspace, size_t workspace_bytes, dg_stream_t stream_) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || h < 1 || w < 1)
        return fail(DG_ERR_INVALID, "dg_augment_forward: B=%d C=%d, image %dx%d, output %dx%d must be positive", B, C, H, W, h, w);
    if (C != 3) return fail(DG_ERR_UNSUPPORTED, "dg_augment_forward: %d channels (the colour ops are RGB: 3)", C);
    if (H < 3 || W < 3 || h < 3 || w < 3)
        return fail(DG_ERR_UNSUPPORTED, "dg_augment_forward: image %dx%d, output %dx%d: reflect padding by 2 needs three pixels a side", H, W, h, w);
    if (B > 65535 || H > 16384 || W > 16384 || h > 16384 || w > 16384)
        return fail(DG_ERR_UNSUPPORTED, "dg_augment_forward: B=%d above 65535 or a side of %dx%d / %dx%d above 16384", B, H, W, h, w);
    if (stride_w != 1 || stride_h != W || stride_c != (int64_t)H * W || stride_b != 3 * (int64_t)H * W)
        return fail(DG_ERR_UNSUPPORTED, "dg_augment_forward: img is not contiguous (strides %lld, %lld, %lld, %lld): copy it once", (long long)stride_b,
                    (long long)stride_c, (long long)stride_h, (long long)stride_w);
    if (!img || !records_host || !params || !img_aug || !coord_aug || !workspace) return fail(DG_ERR_INVALID, "dg_augment_forward: null pointer");
    if (!mean != !stdv) return fail(DG_ERR_INVALID, "dg_augment_forward: mean and std come together: give both or neither");
    if (int rc = check_aligned(__func__, {img, params, img_aug, coord_aug}, workspace)) return rc;
    if (int rc = check_workspace(__func__, workspace_bytes, dg_augment_workspace_bytes(B, h, w), "dg_augment_workspace_bytes")) return rc;
    bool stats = false;
    for (int b = 0; b < B; ++b) {
        const int32_t* r = records_host + (size_t)b * DG_AUGM_REC_WORDS;
        const long long top = r[1], left = r[2], bh = r[3], bw = r[4];
        if (bh < 1 || bw < 1 || top < 0 || left < 0 || top + bh > H || left + bw > W)
            return fail(DG_ERR_UNSUPPORTED, "dg_augment_forward: crop box (%lld, %lld, %lld, %lld) of image %d leaves the %dx%d image", top, left, bh,
                        bw, b, H, W);
        int contrasts = 0;
        for (int k = 0; k < 4; ++k) {
            if (r[5 + k] < -1 || r[5 + k] > DG_AUGM_HUE) return fail(DG_ERR_INVALID, "dg_augment_forward: image %d: op %d in slot %d (-1 .. 3)", b, r[5 + k], k);
            contrasts += r[5 + k] == DG_AUGM_CONTRAST;
        }
        if (contrasts > 1) return fail(DG_ERR_UNSUPPORTED, "dg_augment_forward: image %d has %d contrast ops (one image mean per image: one at most)", b, contrasts);
        float sigma;
        memcpy(&sigma, &r[14], 4);
        if (!(sigma >= 0.f) || std::isinf(sigma)) return fail(DG_ERR_INVALID, "dg_augment_forward: image %d: blur_sigma=%g", b, (double)sigma);
        stats = stats || contrasts > 0;
    }
    DgAugmentArgs A;
    memset(&A, 0, sizeof(A));
    A.img = img;
    A.recs = static_cast<const int32_t*>(params);
    A.rows = reinterpret_cast<const float*>(A.recs + (size_t)B * DG_AUGM_REC_WORDS);
    A.cols = A.rows + H;
    A.img_aug = img_aug; A.coord_aug = coord_aug; A.partials = static_cast<double*>(workspace);
    A.B = B; A.H = H; A.W = W; A.h = h; A.w = w;
    A.tiles_x = (w + DG_AUGM_TW - 1) / DG_AUGM_TW; A.tiles_y = (h + DG_AUGM_TH - 1) / DG_AUGM_TH;
    A.stat_blocks = augment_stat_blocks(h, w);
    A.unit_space = mean ? 0 : 1;
    A.vec_stores = (w % 4 == 0 && (((uintptr_t)img_aug | (uintptr_t)coord_aug) & 15) == 0) ? 1 : 0;
    if (int rc = norm_check(__func__, mean, stdv, A.mean, A.stdv)) return rc;
    DG_HIP(dg_launch_augment(A, stats, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- batch preparation (dg_batch.hip)
extern "C" int dg_batch_prep(const uint8_t* packed, size_t packed_bytes, const int32_t* records_host, const int32_t* tables_host,
                             const void* params, int32_t n_records, int32_t N, int32_t H, int32_t W, const float* mean, const float* stdv,
                             float* img, int64_t* label, void* mask, float* depth, dg_stream_t stream_) {
    if (n_records < 1 || N < 1 || H < 1 || W < 1)
        return fail(DG_ERR_INVALID, "dg_batch_prep: n_records=%d N=%d, output %dx%d must be positive", n_records, N, H, W);
    if (W % 4) return fail(DG_ERR_UNSUPPORTED, "dg_batch_prep: output width %d is not a multiple of 4 (a lane stores four columns as one vector)", W);
    if (H > DG_BATCH_MAX_SIDE || W > DG_BATCH_MAX_SIDE || N > 65535 || n_records > 65535)
        return fail(DG_ERR_UNSUPPORTED, "dg_batch_prep: output %dx%d above %d a side, or N=%d / n_records=%d above 65535", H, W, DG_BATCH_MAX_SIDE, N,
                    n_records);
    if (!records_host || !tables_host || !params || !mean || !stdv) return fail(DG_ERR_INVALID, "dg_batch_prep: null pointer");
    if ((((uintptr_t)img | (uintptr_t)label | (uintptr_t)mask | (uintptr_t)depth) & 15) || ((uintptr_t)params & 3))
        return fail(DG_ERR_INVALID, "dg_batch_prep: img, label, mask and depth must be 16-byte aligned (whole-vector stores), params 4-byte aligned");
    DgBatchArgs A;
    memset(&A, 0, sizeof(A));
    if (int rc = norm_check(__func__, mean, stdv, A.out.mean, A.out.stdv)) return rc;
    // every element of an output is written, and by one record; one mask tensor: one rule
    const PackedSource P = {packed, packed_bytes, records_host, tables_host, params, n_records, H, W};
    int n_out[3], mask_rule = -1;
    if (int rc = walk_records(__func__, P, N, n_out, [&](int i, const int32_t* r, int kind, int n, int out, bool twice) {
            if (out == 0 ? !img : out == 1 ? (!label || !mask) : !depth)
                return fail(DG_ERR_INVALID, "dg_batch_prep: record %d (kind %d) writes an output that is null", i, kind);
            if (twice) return fail(DG_ERR_INVALID, "dg_batch_prep: record %d: sample %d of output %d is written twice", i, n, out);
            if (out != 1) return DG_OK;
            if (r[7] != DG_BATCH_MASK_BOOL_IGNORED && r[7] != DG_BATCH_MASK_FLOAT_POSITIVE)
                return fail(DG_ERR_INVALID, "dg_batch_prep: record %d: unknown mask rule %d (0, 1)", i, r[7]);
            if (mask_rule >= 0 && r[7] != mask_rule)
                return fail(DG_ERR_INVALID, "dg_batch_prep: record %d: mask rule %d after %d (one mask tensor: one rule)", i, r[7], mask_rule);
            mask_rule = r[7];
            return DG_OK;
        }))
        return rc;
    const void* outs[3] = {img, label, depth};
    for (int o = 0; o < 3; ++o)
        if (outs[o] && n_out[o] != N)
            return fail(DG_ERR_INVALID, "dg_batch_prep: output %d has records for %d of %d samples (every element must be written)", o, n_out[o], N);
    A.src = loader_source(P);
    A.out.img = img; A.out.label = reinterpret_cast<long long*>(label); A.out.mask = mask; A.out.depth = depth;
    A.N = N;
    DG_HIP(dg_launch_batch_prep(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- frozen-backbone feature cache (dg_feat_cache.hip)
// what both entries refuse before a launch; `lists`: index lists of n rows each (n * lists blocks along gridDim.y)
static int featcache_check(const char* who, const void* cache, int32_t dtype, int64_t N, int64_t L, int64_t n, int lists) {
    if (dtype < DG_FC_F32 || dtype > DG_FC_BF16) return fail(DG_ERR_INVALID, "%s: unknown dtype %d (0 float32, 1 float16, 2 bfloat16)", who, dtype);
    if (N < 1 || L < 1 || n < 0) return fail(DG_ERR_INVALID, "%s: N=%lld L=%lld n=%lld (N and L positive, n not negative)", who, (long long)N, (long long)L, (long long)n);
    if (n > DG_FC_MAX_ROWS / lists)
        return fail(DG_ERR_UNSUPPORTED, "%s: %d list(s) of %lld rows in one call (at most %d rows)", who, lists, (long long)n, DG_FC_MAX_ROWS);
    if (L > (1ll << 40) || N > (1ll << 62) / L) return fail(DG_ERR_UNSUPPORTED, "%s: a cache of %lld x %lld elements", who, (long long)N, (long long)L);
    if (!cache) return fail(DG_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)cache & (dtype == DG_FC_F32 ? 3 : 1)) return fail(DG_ERR_INVALID, "%s: the cache is not aligned to its element size", who);
    return DG_OK;
}

extern "C" int dg_featcache_put(void* cache, int32_t dtype, int64_t N, int64_t L, const float* src, const int64_t* idx, int64_t n,
                                dg_stream_t stream_) {
    if (int rc = featcache_check(__func__, cache, dtype, N, L, n, 1)) return rc;
    if (n == 0) return DG_OK;
    if (!src || !idx) return fail(DG_ERR_INVALID, "dg_featcache_put: null pointer");
    if (((uintptr_t)src & 3) || ((uintptr_t)idx & 7)) return fail(DG_ERR_INVALID, "dg_featcache_put: src must be 4-byte aligned, idx 8-byte aligned");
    DG_HIP(dg_launch_featcache_put(cache, dtype, N, L, src, reinterpret_cast<const long long*>(idx), (int)n, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_featcache_gather(const void* cache, int32_t dtype, int64_t N, int64_t L, const int64_t* idx_a, const int64_t* idx_b,
                                   int64_t n, float* out, dg_stream_t stream_) {
    if (int rc = featcache_check(__func__, cache, dtype, N, L, n, idx_b ? 2 : 1)) return rc;
    if (n == 0) return DG_OK;
    if (!idx_a || !out) return fail(DG_ERR_INVALID, "dg_featcache_gather: null pointer");
    if (((uintptr_t)out & 3) || (((uintptr_t)idx_a | (uintptr_t)idx_b) & 7))
        return fail(DG_ERR_INVALID, "dg_featcache_gather: out must be 4-byte aligned, idx_a and idx_b 8-byte aligned");
    DG_HIP(dg_launch_featcache_gather(cache, dtype, N, L, reinterpret_cast<const long long*>(idx_a), reinterpret_cast<const long long*>(idx_b),
                                      (int)n, out, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- device-resident sample cache (dg_sample_cache.hip)
// what both entries refuse before a launch; `lists`: index lists of n rows each
static int samplecache_check(const char* who, const void* cache, int64_t n_images, int32_t has_labels, int32_t with_depth, int32_t H, int32_t W,
                             int64_t n, int lists) {
    if (n_images < 1 || H < 1 || W < 1 || n < 0)
        return fail(DG_ERR_INVALID, "%s: n_images=%lld, rows of %dx%d, n=%lld (n_images, H and W positive, n not negative)", who, (long long)n_images, H,
                    W, (long long)n);
    if ((has_labels != 0 && has_labels != 1) || (with_depth != 0 && with_depth != 1))
        return fail(DG_ERR_INVALID, "%s: has_labels=%d with_depth=%d (0 or 1 each)", who, has_labels, with_depth);
    if (W % 4) return fail(DG_ERR_UNSUPPORTED, "%s: row width %d is not a multiple of 4 (a lane moves four columns as one word)", who, W);
    if (H > DG_BATCH_MAX_SIDE || W > DG_BATCH_MAX_SIDE) return fail(DG_ERR_UNSUPPORTED, "%s: rows of %dx%d above %d a side", who, H, W, DG_BATCH_MAX_SIDE);
    if (n > DG_SC_MAX_ROWS / lists)
        return fail(DG_ERR_UNSUPPORTED, "%s: %d list(s) of %lld rows in one call (at most %d rows)", who, lists, (long long)n, DG_SC_MAX_ROWS);
    if (n_images > (1ll << 62) / ((long long)5 * H * W)) return fail(DG_ERR_UNSUPPORTED, "%s: a cache of %lld rows of %dx%d", who, (long long)n_images, H, W);
    if (!cache) return fail(DG_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)cache & 3) return fail(DG_ERR_INVALID, "%s: the cache must be 4-byte aligned (a lane moves four bytes as one word)", who);
    return DG_OK;
}

extern "C" int dg_samplecache_put(uint8_t* cache, int64_t n_images, int32_t has_labels, int32_t with_depth, int32_t H, int32_t W,
                                  const int64_t* idx, int32_t n, const uint8_t* packed, size_t packed_bytes, const int32_t* records_host,
                                  const int32_t* tables_host, const void* params, int32_t n_records, dg_stream_t stream_) {
    if (int rc = samplecache_check(__func__, cache, n_images, has_labels, with_depth, H, W, n, 1)) return rc;
    if (n == 0) return DG_OK;
    if (n_records < 1 || n_records > 65535) return fail(DG_ERR_INVALID, "dg_samplecache_put: n_records=%d outside [1, 65535]", n_records);
    if (!idx || !records_host || !tables_host || !params) return fail(DG_ERR_INVALID, "dg_samplecache_put: null pointer");
    if (((uintptr_t)idx & 7) || ((uintptr_t)params & 3)) return fail(DG_ERR_INVALID, "dg_samplecache_put: idx must be 8-byte aligned, params 4-byte aligned");
    // every byte of every row is written, and by one record
    const PackedSource P = {packed, packed_bytes, records_host, tables_host, params, n_records, H, W};
    int n_out[3];
    if (int rc = walk_records(__func__, P, n, n_out, [&](int i, const int32_t*, int kind, int k, int out, bool twice) {
            if (kind == DG_BATCH_LABEL && !has_labels)
                return fail(DG_ERR_INVALID, "dg_samplecache_put: record %d: sample %d carries a label but the cache has no label plane", i, k);
            if (kind == DG_BATCH_LABEL_FILL && has_labels)
                return fail(DG_ERR_INVALID, "dg_samplecache_put: record %d: sample %d carries no label but the cache has a label plane", i, k);
            if (out == 2 && !with_depth) return fail(DG_ERR_INVALID, "dg_samplecache_put: record %d: sample %d carries depth but the cache has no depth plane", i, k);
            if (twice) return fail(DG_ERR_INVALID, "dg_samplecache_put: record %d: plane group %d of sample %d is written twice", i, out, k);
            return DG_OK;
        }))
        return rc;
    if (n_out[0] != n || (has_labels && n_out[1] != n) || n_out[2] != (with_depth ? n : 0))
        return fail(DG_ERR_INVALID, "dg_samplecache_put: records for %d images, %d labels and %d depth maps of %d samples (every byte of a row must be written)",
                    n_out[0], n_out[1], n_out[2], n);
    DgSampleCachePutArgs A;
    memset(&A, 0, sizeof(A));
    A.cache = cache; A.idx = reinterpret_cast<const long long*>(idx);
    A.src = loader_source(P);
    A.c = cache_planes(n_images, has_labels, with_depth);
    A.n = n;
    DG_HIP(dg_launch_samplecache_put(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

extern "C" int dg_samplecache_gather(const uint8_t* cache, int64_t n_images, int32_t has_labels, int32_t with_depth, int32_t H, int32_t W,
                                     const int64_t* idx_a, const int64_t* idx_b, int32_t n, const float* mean, const float* stdv,
                                     int32_t label_offset, int32_t fill, int32_t mask_rule, float* img, int64_t* label, void* mask, float* depth,
                                     dg_stream_t stream_) {
    if (int rc = samplecache_check(__func__, cache, n_images, has_labels, with_depth, H, W, n, idx_b ? 2 : 1)) return rc;
    if (n == 0) return DG_OK;
    if (!idx_a) return fail(DG_ERR_INVALID, "dg_samplecache_gather: null pointer");
    if (((uintptr_t)idx_a | (uintptr_t)idx_b) & 7) return fail(DG_ERR_INVALID, "dg_samplecache_gather: idx_a and idx_b must be 8-byte aligned");
    if (!img && !label && !mask && !depth) return fail(DG_ERR_INVALID, "dg_samplecache_gather: no output asked for");
    if (((uintptr_t)img | (uintptr_t)label | (uintptr_t)mask | (uintptr_t)depth) & 15)
        return fail(DG_ERR_INVALID, "dg_samplecache_gather: img, label, mask and depth must be 16-byte aligned (whole-vector stores)");
    if (depth && !with_depth) return fail(DG_ERR_INVALID, "dg_samplecache_gather: depth asked of a cache without a depth plane");
    if (mask && mask_rule != DG_BATCH_MASK_BOOL_IGNORED && mask_rule != DG_BATCH_MASK_FLOAT_POSITIVE)
        return fail(DG_ERR_INVALID, "dg_samplecache_gather: unknown mask rule %d (0, 1)", mask_rule);
    DgSampleCacheGatherArgs A;
    memset(&A, 0, sizeof(A));
    if (img) {
        if (!mean || !stdv) return fail(DG_ERR_INVALID, "dg_samplecache_gather: img needs mean and stdv");
        if (int rc = norm_check(__func__, mean, stdv, A.out.mean, A.out.stdv)) return rc;
    }
    A.cache = cache; A.idx_a = reinterpret_cast<const long long*>(idx_a); A.idx_b = reinterpret_cast<const long long*>(idx_b);
    A.out.img = img; A.out.label = reinterpret_cast<long long*>(label); A.out.mask = mask; A.out.depth = depth;
    A.c = cache_planes(n_images, has_labels, with_depth);
    A.n = n; A.H = H; A.W = W;
    A.label_offset = label_offset; A.fill = fill; A.mask_rule = mask_rule;
    DG_HIP(dg_launch_samplecache_gather(A, static_cast<hipStream_t>(stream_)));
    return DG_OK;
}

// ---- the batch draw of a cached step (dg_epoch.hip)
extern "C" int dg_epoch_draw(uint64_t* state, const int64_t* order, const int64_t* nns, int32_t B, int32_t num_neighbors, int64_t n_images,
                             int32_t K, int64_t* ind, int64_t* ind_pos, dg_stream_t stream_) {
    if (B < 1 || n_images < 1 || K < 1)
        return fail(DG_ERR_INVALID, "dg_epoch_draw: B=%d n_images=%lld K=%d must be positive", B, (long long)n_images, K);
    if (num_neighbors < 1 || num_neighbors >= K)
        return fail(DG_ERR_INVALID, "dg_epoch_draw: num_neighbors=%d outside [1, K - 1] of a table with K=%d columns (column 0 is the image itself)",
                    num_neighbors, K);
    if (B > DG_EPOCH_MAX_B) return fail(DG_ERR_UNSUPPORTED, "dg_epoch_draw: B=%d above %d (one block draws the batch)", B, DG_EPOCH_MAX_B);
    if (n_images > (1ll << 62) / K) return fail(DG_ERR_UNSUPPORTED, "dg_epoch_draw: a table of %lld x %d entries", (long long)n_images, K);
    if (!state || !order || !nns || !ind || !ind_pos) return fail(DG_ERR_INVALID, "dg_epoch_draw: null pointer");
    if (((uintptr_t)state | (uintptr_t)order | (uintptr_t)nns | (uintptr_t)ind | (uintptr_t)ind_pos) & 7)
        return fail(DG_ERR_INVALID, "dg_epoch_draw: state, order, nns, ind and ind_pos must be 8-byte aligned");
    // (cursor + B <= n_images cannot be asked here: the cursor lives on the device; the kernel holds its read inside `order`)
    DG_HIP(dg_launch_epoch_draw(reinterpret_cast<unsigned long long*>(state), reinterpret_cast<const long long*>(order),
                                reinterpret_cast<const long long*>(nns), B, num_neighbors, n_images, K, reinterpret_cast<long long*>(ind),
                                reinterpret_cast<long long*>(ind_pos), static_cast<hipStream_t>(stream_)));
    return DG_OK;
}
