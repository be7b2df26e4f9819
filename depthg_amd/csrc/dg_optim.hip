// The optimisation step's three Adams as one launch (reference src/train_segmentation.py:447-455, 537-547: three torch.optim.Adam
// over the head, the cluster probe and the linear probe - nine small fp32 tensors, 205 547 elements at the default configuration):
//   k_adam   torch.optim.Adam's default algorithm (weight_decay = 0, amsgrad = False, maximize = False) over a table of segments
//       exp_avg    = exp_avg + (1 - beta1) * (grad - exp_avg)
//       exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * grad * grad
//       denom      = sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps
//       param      = param - (lr / (1 - beta1^t)) * exp_avg / denom
// The segment table and the groups' scalars are KERNEL ARGUMENTS (by value): in eager mode the gradient pointers change every
// step, a table in device memory would cost a host-to-device copy per step.  Block b works on one chunk of DG_ADAM_CHUNK elements
// of one segment (found through the prefix of chunk counts kept in the table); 128-bit accesses where all four pointers of the
// segment are 16-byte aligned, dwords otherwise (a gradient that is a view into a flat bucket starts at any element).
// Step count: host mode - lr / (1 - beta1^t) and sqrt(1 - beta2^t) arrive as floats, formed on the host in double as torch does;
// device mode - t is a float32 in device memory per segment, one thread of every block forms both corrections from it in double
// (beta^t by squaring: t is a whole number) and the segment's last block to take a ticket stores t + 1.  A block takes its ticket
// after it has read t, so the store cannot overtake a reader; nothing else is handed from block to block, so there is no fence.
// sqrtf and the division are the correctly rounded ones (hipcc's default: no fast-math flag on this file).
#include "dg_device.h"
#include "dg_aux_args.h"

#include <cmath>
#include <cstring>

struct DgAdamKSeg {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* step;            // device mode: the segment's t (float32 scalar); null in host mode
    unsigned int* ticket;   // device mode, segments of more than one chunk: finished-readers counter (zero between launches)
    uint32_t n;             // elements
    uint32_t chunk0;        // first block of the segment (prefix of the chunk counts)
    uint32_t nchunks;
    int32_t group;
    float step_size;        // host mode: lr / (1 - beta1^t)
    float bc2_sqrt;         // host mode: sqrt(1 - beta2^t)
    int32_t vec;            // all four pointers 16-byte aligned
    int32_t pad_;
};
struct DgAdamKGroup {
    double lr, beta1, beta2;      // device mode forms the corrections from these
    float w1, b2, w2, eps;        // (1 - beta1), beta2, (1 - beta2), eps as the floats the update uses
};
struct DgAdamKArgs {
    DgAdamKSeg seg[DG_ADAM_MAX_SEGS];
    DgAdamKGroup grp[DG_ADAM_MAX_GROUPS];
    int32_t n_seg;
};

__device__ __forceinline__ double adam_powi(double b, unsigned int n) {
    double r = 1.0;
    while (n) {
        if (n & 1u) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

__device__ __forceinline__ void adam_one(float g, float& p, float& m, float& v, float w1, float b2, float w2, float eps, float step_size,
                                         float bc2_sqrt) {
    m = m + w1 * (g - m);
    v = b2 * v + w2 * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

template <bool DEVICE_STEPS>
__global__ __launch_bounds__(DG_ADAM_THREADS) void k_adam(const DgAdamKArgs a) {
    int s = 0;
    for (int i = 1; i < a.n_seg; ++i)                 // (uniform: scalar compares on the kernel arguments)
        if (blockIdx.x >= a.seg[i].chunk0) s = i;
    float* __restrict__ p = a.seg[s].p;
    const float* __restrict__ g = a.seg[s].g;
    float* __restrict__ m = a.seg[s].m;
    float* __restrict__ v = a.seg[s].v;
    const uint32_t n = a.seg[s].n;
    const int gi = a.seg[s].group;
    const float w1 = a.grp[gi].w1, b2 = a.grp[gi].b2, w2 = a.grp[gi].w2, eps = a.grp[gi].eps;
    float step_size = a.seg[s].step_size, bc2_sqrt = a.seg[s].bc2_sqrt;
    if (DEVICE_STEPS) {
        __shared__ float corr[2];
        float* step = a.seg[s].step;
        unsigned int* ticket = a.seg[s].ticket;
        const uint32_t nchunks = a.seg[s].nchunks;
        float t_new = 0.f;
        if (threadIdx.x == 0) {
            t_new = __hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1.0f;
            const unsigned int t = (unsigned int)t_new;
            corr[0] = (float)(a.grp[gi].lr / (1.0 - adam_powi(a.grp[gi].beta1, t)));
            corr[1] = (float)sqrt(1.0 - adam_powi(a.grp[gi].beta2, t));
        }
        __syncthreads();
        step_size = corr[0];
        bc2_sqrt = corr[1];
        if (threadIdx.x == 0) {
            // t has been read (its value went into corr[]): take the ticket; the last reader of the segment advances t
            bool last = true;
            if (nchunks > 1) {
                last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nchunks - 1;
                if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (last) __hip_atomic_store(step, t_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const uint32_t base = (blockIdx.x - a.seg[s].chunk0) * DG_ADAM_CHUNK;
    const uint32_t i = base + threadIdx.x * 4;                    // DG_ADAM_CHUNK = 4 * DG_ADAM_THREADS
    if (a.seg[s].vec && i + 4 <= n) {
        const float4 g4 = *reinterpret_cast<const float4*>(g + i);
        float4 p4 = *reinterpret_cast<const float4*>(p + i);
        float4 m4 = *reinterpret_cast<const float4*>(m + i);
        float4 v4 = *reinterpret_cast<const float4*>(v + i);
        adam_one(g4.x, p4.x, m4.x, v4.x, w1, b2, w2, eps, step_size, bc2_sqrt);
        adam_one(g4.y, p4.y, m4.y, v4.y, w1, b2, w2, eps, step_size, bc2_sqrt);
        adam_one(g4.z, p4.z, m4.z, v4.z, w1, b2, w2, eps, step_size, bc2_sqrt);
        adam_one(g4.w, p4.w, m4.w, v4.w, w1, b2, w2, eps, step_size, bc2_sqrt);
        *reinterpret_cast<float4*>(p + i) = p4;
        *reinterpret_cast<float4*>(m + i) = m4;
        *reinterpret_cast<float4*>(v + i) = v4;
    } else if (a.seg[s].vec) {                                    // the tail of an aligned segment: < 4 elements
        for (uint32_t j = i; j < n; ++j) {
            float pj = p[j], mj = m[j], vj = v[j];
            adam_one(g[j], pj, mj, vj, w1, b2, w2, eps, step_size, bc2_sqrt);
            p[j] = pj; m[j] = mj; v[j] = vj;
        }
    } else {                                                      // dword path: lane-contiguous, four rounds per chunk
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t j = base + r * DG_ADAM_THREADS + threadIdx.x;
            if (j < n) {
                float pj = p[j], mj = m[j], vj = v[j];
                adam_one(g[j], pj, mj, vj, w1, b2, w2, eps, step_size, bc2_sqrt);
                p[j] = pj; m[j] = mj; v[j] = vj;
            }
        }
    }
}

hipError_t dg_launch_adam(const dg_adam_seg* segs, int n_seg, const dg_adam_group* groups, int n_groups, bool device_steps,
                          unsigned int* tickets, hipStream_t s) {
    DgAdamKArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < n_groups; ++k) {
        const double b1 = groups[k].beta1, b2 = groups[k].beta2;
        a.grp[k].lr = groups[k].lr; a.grp[k].beta1 = b1; a.grp[k].beta2 = b2;
        a.grp[k].w1 = (float)(1.0 - b1); a.grp[k].b2 = (float)b2; a.grp[k].w2 = (float)(1.0 - b2); a.grp[k].eps = (float)groups[k].eps;
    }
    uint32_t chunks = 0;
    int n = 0;
    for (int k = 0; k < n_seg; ++k) {
        const dg_adam_seg& h = segs[k];
        if (!h.grad) continue;                        // torch skips parameters whose .grad is None: state and t untouched
        DgAdamKSeg& d = a.seg[n++];
        d.p = h.param; d.g = h.grad; d.m = h.exp_avg; d.v = h.exp_avg_sq;
        d.step = device_steps ? h.step_dev : nullptr;
        d.ticket = device_steps && tickets ? tickets + k : nullptr;
        d.n = (uint32_t)h.numel;
        d.chunk0 = chunks;
        d.nchunks = (uint32_t)((h.numel + DG_ADAM_CHUNK - 1) / DG_ADAM_CHUNK);
        d.group = h.group;
        if (!device_steps) {                          // torch/optim/adam.py _single_tensor_adam: Python floats, i.e. double
            const dg_adam_group& gr = groups[h.group];
            d.step_size = (float)(gr.lr / (1.0 - pow(gr.beta1, h.step_host)));
            d.bc2_sqrt = (float)sqrt(1.0 - pow(gr.beta2, h.step_host));
        }
        d.vec = (((uintptr_t)h.param | (uintptr_t)h.grad | (uintptr_t)h.exp_avg | (uintptr_t)h.exp_avg_sq) & 15) == 0;
        chunks += d.nchunks;
    }
    if (n == 0) return hipSuccess;
    a.n_seg = n;
    if (device_steps) hipLaunchKernelGGL(k_adam<true>, dim3(chunks), dim3(DG_ADAM_THREADS), 0, s, a);
    else hipLaunchKernelGGL(k_adam<false>, dim3(chunks), dim3(DG_ADAM_THREADS), 0, s, a);
    return hipGetLastError();
}
