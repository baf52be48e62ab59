// s2d_raster_det.hip -- deterministic mode's gather kernels: the fixed-order sums of the slots that the backward walks of the
// other raster units stored their partial gradients (and density statistics) into.
#include "s2d_walk_backward.h"

namespace s2d {

// Deterministic mode: gradient of splat i = sum of the partials its tiles stored this iteration, in emission
// (tile row-major) order -- the same order whatever the dispatch order of the tiles was.  A splat's tiles announce
// themselves in touched[i] (bit j = its j-th emission slot; a tile reaches a splat's entry only while some pixel of it is
// still live, so most of a splat's ~20 slots stay unwritten and a hidden splat has none): the pass reads one word per
// splat and then only the slots that hold something, instead of every stamp of every slot.  Slots from the 32nd on share
// bit 31 and are told apart by their stamps.  The word is cleared for the next pass.
__device__ __forceinline__ void det_add_slot(float (&acc)[9], const float* __restrict__ data, uint32_t slot)
{
    const float4* d = reinterpret_cast<const float4*>(data + (size_t)slot * kDetStride); // three 16-byte loads per slot
    const float4 a = d[0], b = d[1], c = d[2];
    acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
    acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
    acc[8] += c.x;
}

__global__ __launch_bounds__(256) void gather_grads_kernel(const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ counts, int n,
                                                           const float* __restrict__ data,
                                                           const uint32_t* __restrict__ stamp, uint32_t* __restrict__ touched,
                                                           uint32_t now, float* __restrict__ grads)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t m = touched[i];
    if (m == 0u) return; // no tile wrote anything for this splat: its gradient record stays as it is (zero)
    touched[i] = 0u;
    float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const uint32_t o = offsets[i];
    const bool tail = (m >> 31) != 0u;
    m &= 0x7FFFFFFFu;
    while (m != 0u) { // ascending slot order, four slots' loads in flight at a time
        uint32_t js[4];
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (m != 0u) {
                js[q] = (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
                cnt = q + 1;
            }
        float4 v[4][3];
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < cnt) {
                const float4* d = reinterpret_cast<const float4*>(data + (size_t)(o + js[q]) * kDetStride);
                v[q][0] = d[0]; v[q][1] = d[1]; v[q][2] = d[2];
            }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < cnt) {
                acc[0] += v[q][0].x; acc[1] += v[q][0].y; acc[2] += v[q][0].z; acc[3] += v[q][0].w;
                acc[4] += v[q][1].x; acc[5] += v[q][1].y; acc[6] += v[q][1].z; acc[7] += v[q][1].w;
                acc[8] += v[q][2].x;
            }
    }
    if (tail) {
        const uint32_t c = counts[i];
        for (uint32_t s = o + 31u; s < o + c; s++)
            if (stamp[s] == now) det_add_slot(acc, data, s);
    }
    float* gr = grads + (size_t)i * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) gr[k] += acc[k]; // += : the buffer is zero here unless the caller accumulates slabs
}

// Deterministic mode, density statistics: words 9..11 of the same slots, in the same order, into stats[i] (n x 3, accumulated
// over passes).  Runs BEFORE gather_grads_kernel, which clears the `touched` words both read: the statistics ride in the
// gradient slots of their own pass, so a slot is read here exactly when that pass wrote all twelve of its words.
__global__ __launch_bounds__(256) void gather_stats_kernel(const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ counts, int n,
                                                           const float* __restrict__ data,
                                                           const uint32_t* __restrict__ stamp,
                                                           const uint32_t* __restrict__ touched, uint32_t now,
                                                           float* __restrict__ stats)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t m = touched[i];
    if (m == 0u) return;
    float acc[3] = {0.f, 0.f, 0.f};
    const uint32_t o = offsets[i];
    const bool tail = (m >> 31) != 0u;
    m &= 0x7FFFFFFFu;
    while (m != 0u) { // ascending slot order
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        const float4 c = reinterpret_cast<const float4*>(data + (size_t)(o + j) * kDetStride)[2];
        acc[0] += c.y; acc[1] += c.z; acc[2] += c.w;
    }
    if (tail) {
        const uint32_t cnt = counts[i];
        for (uint32_t s = o + 31u; s < o + cnt; s++)
            if (stamp[s] == now) {
                const float4 c = reinterpret_cast<const float4*>(data + (size_t)s * kDetStride)[2];
                acc[0] += c.y; acc[1] += c.z; acc[2] += c.w;
            }
    }
    float* st = stats + (size_t)i * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) st[k] += acc[k];
}

// Behind every backward walk.  Deterministic mode (a.det.now != 0): the statistics of a STATS walk (a.density) first, then the
// gradients.  Returns the status of the pass's launches, the walk before it included.
hipError_t launch_det_gather(const RasterArgs& a, hipStream_t stream)
{
    const DetGather& dg = a.det;
    if (dg.now != 0u && dg.n > 0) {
        if (a.density != nullptr)
            hipLaunchKernelGGL(gather_stats_kernel, dim3((dg.n + 255) / 256), dim3(256), 0, stream, dg.offsets, dg.counts, dg.n,
                               dg.data, dg.stamp, dg.touched, dg.now, a.density);
        hipLaunchKernelGGL(gather_grads_kernel, dim3((dg.n + 255) / 256), dim3(256), 0, stream, dg.offsets, dg.counts, dg.n,
                           dg.data, dg.stamp, dg.touched, dg.now, a.grads);
    }
    return hipGetLastError();
}

} // namespace s2d
