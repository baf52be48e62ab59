// s2d_alive.hip -- the kernels of the alive set (s2d_alive.h).  Rare, host-driven calls over n rows:
// each kernel is one thread per row, bounds-checked against n, reading and writing bytes and words of its own row only.
#include "s2d_alive.h"

namespace s2d {

__global__ __launch_bounds__(256) void alive_flags_kernel(const uint8_t* src, int invert, int n, uint8_t* held,
                                                          uint32_t* __restrict__ flags, float* __restrict__ grads)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = ((src[i] != 0) != (invert != 0)) ? 1u : 0u; // (src may be held: read before the write below)
    if (held) held[i] = (uint8_t)f;
    flags[i] = f;
    if (grads && f == 0u) {
        float* gr = grads + (size_t)i * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) gr[k] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void alive_prune_kernel(uint8_t* __restrict__ held, const float* __restrict__ stats,
                                                          const float* __restrict__ splats, int n, int passes, float min_weight,
                                                          float min_opacity)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (held[i] == 0) return;
    bool prune = false;
    if (min_weight > 0.0f) prune = (double)stats[(size_t)i * 3 + 2] / (double)passes < (double)min_weight;
    if (min_opacity > 0.0f) prune = prune || splats[(size_t)i * 9 + 8] < min_opacity;
    if (prune) held[i] = 0;
}

__global__ __launch_bounds__(256) void alive_pick_dead_kernel(uint8_t* __restrict__ held, const uint32_t* __restrict__ pos, int n,
                                                              uint32_t limit, int32_t* __restrict__ ids_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (held[i] != 0) return;
    const uint32_t p = pos[i]; // the number of dead rows below i: < n, and < limit <= the capacity of ids_out where it is used
    if (p >= limit) return;
    ids_out[p] = i;
    held[i] = 1;
}

hipError_t launch_alive_flags(const uint8_t* src, int invert, int n, uint8_t* held, uint32_t* flags, float* grads, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(alive_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, invert, n, held, flags, grads);
    return hipGetLastError();
}

hipError_t launch_alive_prune(const AlivePruneArgs& a, hipStream_t stream)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(alive_prune_kernel, dim3((a.n + 255) / 256), dim3(256), 0, stream, a.held, a.stats, a.splats, a.n, a.passes,
                       a.min_weight, a.min_opacity);
    return hipGetLastError();
}

hipError_t launch_alive_pick_dead(uint8_t* held, const uint32_t* pos, int n, uint32_t limit, int32_t* ids_out, hipStream_t stream)
{
    if (n <= 0 || limit == 0u) return hipSuccess;
    hipLaunchKernelGGL(alive_pick_dead_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, held, pos, n, limit, ids_out);
    return hipGetLastError();
}

} // namespace s2d
