// The batch draw of a cached training step, on the device (reference src/data.py:1073-1080: the loader hands out dataset index `ind`
// and draws its positive as nns[ind][torch.randint(1, num_neighbors + 1)], one host draw per sample).
//   k_epoch_draw  slot j of a batch of B: ind[j] = order[cursor + j], ind_pos[j] = nns[ind[j]][1 + u_j % num_neighbors] with u_j the
//                 first word of Philox4x32-10 keyed by `seed` at the 64-bit counter draws + j; then cursor += B and draws += B.
// seed, draws and cursor are READ FROM THE DEVICE (state = {seed, draws, cursor}, three 64-bit words): nothing about a draw is a
// kernel argument, so a launch recorded in a hipGraph draws the next batch at every replay, as k_rand_coords_state does for the
// step's coordinates.  One block of up to DG_EPOCH_MAX_B threads: the state words are read by every thread, the barrier stands
// between those reads and the one thread that advances them.  No LDS, no atomics; every element of ind and ind_pos is written, with
// plain vector stores.  The position in `order` is held inside [0, n_images) (the caller keeps cursor + B <= n_images; a broken
// invariant then repeats the last entry instead of reading past the buffer), and so is the table row formed from order's value.
#include "dg_device.h"
#include "dg_data_args.h"

__global__ __launch_bounds__(DG_EPOCH_MAX_B) void k_epoch_draw(unsigned long long* __restrict__ state, const long long* __restrict__ order,
                                                               const long long* __restrict__ nns, int B, int num_neighbors, long long n_images,
                                                               int K, long long* __restrict__ ind, long long* __restrict__ ind_pos) {
    const int j = threadIdx.x;
    const unsigned long long seed = state[0], draws = state[1], cursor = state[2];
    if (j < B) {
        const unsigned long long at = cursor + (unsigned long long)j;                                  // (a negative cursor is a huge one)
        const long long image = order[at < (unsigned long long)n_images ? at : (unsigned long long)(n_images - 1)];
        const long long row = image < 0 ? 0 : (image >= n_images ? n_images - 1 : image);
        const unsigned long long ctr = draws + (unsigned long long)j;
        const uint32_t u = dg_philox4(seed, (uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u)[0];
        const int r = 1 + (int)(u % (uint32_t)num_neighbors);                                          // 1 .. num_neighbors < K
        ind[j] = image;
        ind_pos[j] = nns[(size_t)row * K + r];
    }
    __syncthreads();                                            // (every thread of the block has read the state)
    if (j == 0) {
        state[1] = draws + (unsigned long long)B;
        state[2] = cursor + (unsigned long long)B;
    }
}

hipError_t dg_launch_epoch_draw(unsigned long long* state, const long long* order, const long long* nns, int B, int num_neighbors,
                                long long n_images, int K, long long* ind, long long* ind_pos, hipStream_t s) {
    const int threads = (B + 63) / 64 * 64;                     // whole waves, B <= DG_EPOCH_MAX_B
    hipLaunchKernelGGL(k_epoch_draw, dim3(1), dim3(threads), 0, s, state, order, nns, B, num_neighbors, n_images, K, ind, ind_pos);
    return hipGetLastError();
}
