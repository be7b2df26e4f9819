// The last launch of the three auxiliary loss terms' forwards (dg_crf_loss.hip, dg_aug.hip, dg_rec_loss.hip): their blocks each leave
// one fp64 partial sum in the workspace, and one block turns the partials into the loss scalar.
#include "dg_loss_args.h"

// loss = scale * sum of the partial sums, in fp64 and in one fixed order.  grid 1, block 256.
__global__ __launch_bounds__(256) void k_loss_reduce(const double* part, int np, double scale, float* loss) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) s += part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(sh[0] * scale);
}

hipError_t dg_launch_loss_reduce(const double* part, int np, double scale, float* loss, hipStream_t s) {
    hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(256), 0, s, part, np, scale, loss);
    return hipGetLastError();
}
