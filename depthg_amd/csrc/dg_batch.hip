// Batch preparation (depthg_amd/data.py): the loader transform of the training data path for a whole batch - the samples and their
// kNN positives - in ONE launch.  The reference's get_transform (src/utils.py:164-182) is
//     Resize(res, NEAREST) -> cropper -> ToTensor -> Normalize      on the image
//     Resize(res, NEAREST) -> cropper -> ToTargetTensor             on the label and the depth map
// per sample on the CPU: a gather per output pixel, then two float32 operations.  Here the decoded uint8 planes of all samples lie in
// one packed device buffer, every source at its own size; the resize and the crop are composed on the host into two index tables
// per sample (xs[W]: the source column of every output column, ys[H]: the source row of every output row), and a record per output
// plane group says where the source lies and what to write:
//     image        (N,3,H,W) float32  (byte / 255 - mean[c]) / std[c]      ToTensor's division, then Normalize's sub and div
//     label        (N,H,W)   int64    byte + label_offset                    and the mask: bool (label == -1) or float32 (label > 0)
//     depth        (N,H,W)   float32  the byte value; the plane variant and the constant label read no source
// Output-stationary: grid (tiles of 16 rows x 64 columns, records), one lane per four neighbouring output columns of a row.  The
// block's 16 row indices and 64 column indices are read once into LDS (dg_tile_prologue of dg_data_args.h, which k_sc_put opens with
// too); a lane gathers its four bytes of a plane as one word (dg_gather4) and hands it to the writers k_sc_gather forms its outputs
// with (dg_write_image, dg_write_label, dg_write_depth): every float32 and int64 store is a whole 16-byte vector (the byte mask's
// four columns are one 4-byte word).  W is a multiple of 4 and every output 16-byte aligned: the host entry refuses
// anything else, so no lane has a partial vector.  No atomics, no intermediate image; each output element is written by exactly one
// lane of one record (the host entry checks that the records cover every sample once), so two calls give the same bytes.
// Arithmetic: float32 with IEEE division and no contraction - the bits of torch's CPU chain.
// The records and tables are device data: the host entry has checked a host copy, and the kernel still holds every index inside
// its plane.
#include "dg_data_args.h"
#include "dg_device.h"

#pragma clang fp contract(off)

// grid (tiles_x * tiles_y, n_records), block 256, 320 bytes of LDS.
__global__ __launch_bounds__(DG_BATCH_THREADS) void k_batch_prep(DgBatchArgs A) {
    __shared__ int s_x[DG_BATCH_TW], s_y[DG_BATCH_TH];
    const DgRecord R = dg_record(A.src.recs, blockIdx.y);
    const bool reads = R.kind == DG_BATCH_IMAGE || R.kind == DG_BATCH_LABEL || R.kind == DG_BATCH_DEPTH;
    const DgTileLane L = dg_tile_prologue(A.src, R, reads, s_x, s_y);
    if (!L.owns) return;
    const size_t oplane = (size_t)A.src.H * A.src.W, pix = (size_t)L.oy * A.src.W + L.ox, opix = (size_t)R.sample * oplane + pix;

    if (R.kind == DG_BATCH_IMAGE) {
        uint32_t word[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) word[c] = dg_gather4(A.src, R, s_x, s_y, L, 3, c);
        dg_write_image(A.out.img + (size_t)R.sample * 3 * oplane + pix, oplane, word, A.out.mean, A.out.stdv);
    } else if (R.kind == DG_BATCH_LABEL || R.kind == DG_BATCH_LABEL_FILL) {
        long long lab[4] = {R.label_offset, R.label_offset, R.label_offset, R.label_offset};
        if (R.kind == DG_BATCH_LABEL) dg_labels(dg_gather4(A.src, R, s_x, s_y, L), R.label_offset, lab);
        dg_write_label(A.out.label, A.out.mask, opix, R.mask_rule, lab);
    } else if (R.kind == DG_BATCH_DEPTH || R.kind == DG_BATCH_DEPTH_PLANE) {
        dg_write_depth(A.out.depth + opix, R.kind == DG_BATCH_DEPTH ? dg_gather4(A.src, R, s_x, s_y, L) : 0xffffffffu);      // the plane: 255
    }
}

hipError_t dg_launch_batch_prep(const DgBatchArgs& A, hipStream_t s) {
    return dg_launch_if(false, k_batch_prep, dim3(A.src.tiles_x * A.src.tiles_y, A.src.n_records), dim3(DG_BATCH_THREADS), 0, s, A);
}
