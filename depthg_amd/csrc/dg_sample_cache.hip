// Device-resident sample cache (depthg_amd/sample_cache.py).  With a deterministic loader crop the resized and cropped bytes of every
// image, label and depth map (src/utils.py:164-182) are the same in every epoch, and so is everything the reference's datasets form
// from them (src/data.py:894-902, :126-128).  The cache keeps those bytes on the card as uint8 (n_images, planes, H, W) at the
// loader's OUTPUT size - planes R, G, B, then the label if the dataset has labels, then the depth if it is wanted - and a batch and
// its kNN positives come back in the step's dtypes from one launch, with no file, no decoder, no pinned buffer and no upload.  Both
// kernels stand on the prologue and writers of dg_data_args.h, which k_batch_prep stands on too:
//   k_sc_put     rows idx[0..n) of the cache = the bytes the loader's nearest resize and crop select from the packed source planes:
//                dg_tile_prologue and dg_gather4 under dg_batch_prep's records and tables, the words stored as they are.  Image HWC
//                becomes three planes; a DG_BATCH_DEPTH_PLANE record stores the byte 255 (float(255) is what k_batch_prep writes for
//                that kind); a DG_BATCH_LABEL_FILL record writes nothing (such a cache has no label plane).  A lane owns four
//                neighbouring columns of a row and stores them as one 32-bit word per plane.
//   k_sc_gather  rows 0..n-1 from idx_a, rows n..2n-1 from idx_b (null: n rows), each output that is not null:
//                    img   fp32  dg_write_image
//                    label int64 byte + label_offset, or `fill` without a label plane; mask fp32 label > 0, or a bool byte
//                                label == -1 (dg_labels, dg_write_label)
//                    depth fp32 the byte (dg_write_depth)
//                A plane of a row is H W contiguous bytes, so the lanes walk it flat: lane k of a row owns pixels 4k .. 4k + 3, loads
//                them as ONE 32-bit word per plane (W % 4 == 0 and a 4-byte aligned cache keep every word aligned) and stores 16-byte
//                vectors - a wave's store of a float plane is 1 KiB contiguous - and the bool mask as one 4-byte word.
// No atomics; every byte of every row a put names and every element of every gathered output is written by exactly one lane, so two
// calls give the same bytes.  The row index is read from device memory by every block of the row; one outside [0, n_images) ends the
// block before an address is formed from it.
#include "dg_data_args.h"
#include "dg_device.h"

#pragma clang fp contract(off)

// grid (tiles_x * tiles_y, n_records), block 256, 320 bytes of LDS.
__global__ __launch_bounds__(DG_BATCH_THREADS) void k_sc_put(DgSampleCachePutArgs A) {
    __shared__ int s_x[DG_BATCH_TW], s_y[DG_BATCH_TH];
    const DgRecord R = dg_record(A.src.recs, blockIdx.y);
    const int plane = R.kind == DG_BATCH_IMAGE ? 0 : R.kind == DG_BATCH_LABEL ? A.c.label_plane
                    : (R.kind == DG_BATCH_DEPTH || R.kind == DG_BATCH_DEPTH_PLANE) ? A.c.depth_plane : -1;
    if (plane < 0 || R.sample < 0 || R.sample >= A.n) return;       // (the record is uniform over the block: so are this and the prologue's barrier)
    const long long row = A.idx[R.sample];
    if (row < 0 || row >= A.c.n_images) return;
    const DgTileLane L = dg_tile_prologue(A.src, R, R.kind != DG_BATCH_DEPTH_PLANE, s_x, s_y);
    if (!L.owns) return;
    const size_t oplane = (size_t)A.src.H * A.src.W;
    uint8_t* dst = A.cache + ((size_t)row * A.c.planes + plane) * oplane + (size_t)L.oy * A.src.W + L.ox;

    if (R.kind == DG_BATCH_IMAGE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(dst + c * oplane) = dg_gather4(A.src, R, s_x, s_y, L, 3, c);
    } else {                                        // DG_BATCH_DEPTH_PLANE: four bytes 255
        *reinterpret_cast<uint32_t*>(dst) = R.kind != DG_BATCH_DEPTH_PLANE ? dg_gather4(A.src, R, s_x, s_y, L) : 0xffffffffu;
    }
}

// grid (ceil(H W / 4 / 256), rows), block 256.
__global__ __launch_bounds__(DG_SC_THREADS) void k_sc_gather(DgSampleCacheGatherArgs A) {
    const int j = blockIdx.y;
    const long long row = j < A.n ? A.idx_a[j] : A.idx_b[j - A.n];
    if (row < 0 || row >= A.c.n_images) return;
    const size_t oplane = (size_t)A.H * A.W;
    const size_t q = ((size_t)blockIdx.x * DG_SC_THREADS + threadIdx.x) * 4;
    if (q >= oplane) return;                        // H W % 4 == 0: a lane has its four pixels or none
    const uint8_t* src = A.cache + (size_t)row * A.c.planes * oplane + q;
    const size_t opix = (size_t)j * oplane + q;

    if (A.out.img) {
        uint32_t word[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) word[c] = *reinterpret_cast<const uint32_t*>(src + c * oplane);      // (the three loads are in flight together)
        dg_write_image(A.out.img + (size_t)j * 3 * oplane + q, oplane, word, A.out.mean, A.out.stdv);
    }
    if (A.out.label || A.out.mask) {
        long long lab[4] = {A.fill, A.fill, A.fill, A.fill};
        if (A.c.label_plane >= 0) dg_labels(*reinterpret_cast<const uint32_t*>(src + (size_t)A.c.label_plane * oplane), A.label_offset, lab);
        dg_write_label(A.out.label, A.out.mask, opix, A.mask_rule, lab);
    }
    if (A.out.depth) dg_write_depth(A.out.depth + opix, *reinterpret_cast<const uint32_t*>(src + (size_t)A.c.depth_plane * oplane));
}

hipError_t dg_launch_samplecache_put(const DgSampleCachePutArgs& A, hipStream_t s) {
    return dg_launch_if(false, k_sc_put, dim3(A.src.tiles_x * A.src.tiles_y, A.src.n_records), dim3(DG_BATCH_THREADS), 0, s, A);
}

hipError_t dg_launch_samplecache_gather(const DgSampleCacheGatherArgs& A, hipStream_t s) {
    const size_t lanes = ((size_t)A.H * A.W) / 4;
    const int rows = A.idx_b ? 2 * A.n : A.n;
    return dg_launch_if(false, k_sc_gather, dim3((unsigned)((lanes + DG_SC_THREADS - 1) / DG_SC_THREADS), (unsigned)rows), dim3(DG_SC_THREADS),
                        0, s, A);
}
