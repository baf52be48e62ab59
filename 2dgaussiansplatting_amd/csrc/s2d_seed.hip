// s2d_seed.hip -- the importance map, its prefix sums and the sampler on the device (s2d_seed.h).
//
// A map is two launches, a placement a third:
//   seed_importance_kernel  one workgroup per share of 1024 consecutive pixels (the shape of loss_pointwise_kernel): wave w
//                           loads chunk 4 k + w in its k-th round, one 16-byte (8-byte with fp16 images) load per lane and
//                           image; stores q of every pixel and the sum of every chunk.
//   seed_scan_kernel        one workgroup: thread t owns the shares [t * per, (t + 1) * per), adds their chunk sums, the 256
//                           thread sums are scanned by a fixed tree in LDS, and the thread writes its shares' inclusive 64-bit
//                           prefixes.
//   seed_place_kernel       one thread per row: the two draws, a binary search over the share prefixes, the walk over the
//                           share's 16 chunk sums and the chunk's 64 pixels, the target's colour, 9 + 18 floats.
// No atomics: every word has one writer; the sums are integers, so no order is involved either.
#include "s2d_seed.h"

#include <hip/hip_fp16.h>

#include "s2d_seed_math.h"

namespace s2d {

template <bool HALF>
__device__ __forceinline__ void seed_load_rgb(const void* base, size_t i, float* rgb)
{
    if (HALF) {
        const uint2 v = reinterpret_cast<const uint2*>(base)[i];
        const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&v.x));
        const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&v.y));
        rgb[0] = a.x, rgb[1] = a.y, rgb[2] = b.x;
    } else {
        const float4 v = reinterpret_cast<const float4*>(base)[i];
        rgb[0] = v.x, rgb[1] = v.y, rgb[2] = v.z;
    }
}

template <int SOURCE, bool HALF>
__global__ __launch_bounds__(256) void seed_importance_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                              const float* __restrict__ caller, int W, int H, size_t pixels,
                                                              int squared, uint32_t floor_q, uint32_t* __restrict__ q,
                                                              uint32_t* __restrict__ chunk_sum)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < kSeedChunks / 4; k++) {
        const int chunk = 4 * k + wave;
        const size_t i = (size_t)blockIdx.x * kSeedShare + (size_t)chunk * kSeedChunk + (size_t)lane;
        uint32_t v = 0;
        if (i < pixels) {
            float s;
            if (SOURCE == (int)SeedSource::TargetEdges) {
                const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * (size_t)W);
                const size_t row = (size_t)y * (size_t)W;
                const size_t il = row + (size_t)(x > 0 ? x - 1 : 0), ir = row + (size_t)(x < W - 1 ? x + 1 : W - 1);
                const size_t iu = (size_t)(y > 0 ? y - 1 : 0) * (size_t)W + (size_t)x;
                const size_t id = (size_t)(y < H - 1 ? y + 1 : H - 1) * (size_t)W + (size_t)x;
                float l[3], r[3], u[3], d[3];
                seed_load_rgb<HALF>(image_ref, il, l);
                seed_load_rgb<HALF>(image_ref, ir, r);
                seed_load_rgb<HALF>(image_ref, iu, u);
                seed_load_rgb<HALF>(image_ref, id, d);
                s = seed_measure_edges(l, r, u, d);
            } else if (SOURCE == (int)SeedSource::Error) {
                float a[3], b[3];
                seed_load_rgb<HALF>(image0, i, a);
                seed_load_rgb<HALF>(image_ref, i, b);
                s = seed_measure_error(a, b);
            } else {
                s = seed_measure_caller(caller[i]);
            }
            v = seed_quantise(s, squared != 0, floor_q);
            q[i] = v;
        }
        // the chunk's sum: a pixel beyond the image counts 0 (every lane of the wave is here)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0) chunk_sum[(size_t)blockIdx.x * kSeedChunks + chunk] = v;
    }
}

__global__ __launch_bounds__(256) void seed_scan_kernel(const uint32_t* __restrict__ chunk_sum, size_t shares,
                                                        uint64_t* __restrict__ share_prefix)
{
    __shared__ uint64_t part[256];
    const size_t per = (shares + 255) / 256;
    const size_t first = (size_t)threadIdx.x * per, last = first + per < shares ? first + per : shares;
    uint64_t mine = 0;
    for (size_t s = first; s < last; s++) {
        uint32_t v = 0;
#pragma unroll
        for (int c = 0; c < kSeedChunks; c++) v += chunk_sum[s * kSeedChunks + c]; // <= 1024 * 8190
        mine += v;
    }
    part[threadIdx.x] = mine;
    __syncthreads();
    // inclusive scan of the 256 thread sums (Hillis-Steele, 8 rounds)
    for (int d = 1; d < 256; d <<= 1) {
        const uint64_t add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - mine; // everything before this thread's shares
    for (size_t s = first; s < last; s++) {
        uint32_t v = 0;
#pragma unroll
        for (int c = 0; c < kSeedChunks; c++) v += chunk_sum[s * kSeedChunks + c];
        run += v;
        share_prefix[s] = run;
    }
}

__global__ __launch_bounds__(256) void seed_place_kernel(SeedPlaceArgs a)
{
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= a.count) return;
    const uint32_t row = a.ids ? (uint32_t)a.ids[j] : (uint32_t)j;
    const SeedDraw dr = seed_draw(row, a.seed, a.total);
    // the first share whose inclusive prefix exceeds u (u < total = the last prefix)
    size_t lo = 0, hi = a.map.shares - 1;
    while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        if (a.map.share_prefix[mid] > dr.u) hi = mid;
        else lo = mid + 1;
    }
    uint64_t rem = dr.u - (lo > 0 ? a.map.share_prefix[lo - 1] : 0ull); // < the share's sum
    int chunk = 0;
    for (; chunk < kSeedChunks - 1; chunk++) {
        const uint32_t v = a.map.chunk_sum[lo * kSeedChunks + chunk];
        if (rem < v) break;
        rem -= v;
    }
    const size_t base = lo * kSeedShare + (size_t)chunk * kSeedChunk;
    const size_t left = base < a.map.pixels ? a.map.pixels - base : 1; // pixels of the chunk inside the image (>= 1 where a draw can land)
    const int len = left < (size_t)kSeedChunk ? (int)left : kSeedChunk;
    int k = 0;
    for (; k < len - 1; k++) {
        const uint32_t v = a.map.q[base + k];
        if (rem < v) break;
        rem -= v;
    }
    size_t p = base + (size_t)k;
    if (p >= a.map.pixels) p = a.map.pixels - 1; // (never taken with a consistent map: keeps every access inside the image)
    const int y = (int)(p / (size_t)a.W), x = (int)(p - (size_t)y * (size_t)a.W);
    float rgb[3];
    if (a.half_images) seed_load_rgb<true>(a.image_ref, p, rgb);
    else seed_load_rgb<false>(a.image_ref, p, rgb);
    float out[9];
    seed_row(x, y, dr, a.W, a.H, a.scale, a.opacity, rgb, out);
    float* s = a.splats + (size_t)row * 9;
#pragma unroll
    for (int c = 0; c < 9; c++) s[c] = out[c];
    float* m = a.adams + (size_t)row * 18;
#pragma unroll
    for (int c = 0; c < 18; c++) m[c] = 0.0f;
}

template <int SOURCE>
static void launch_importance(const SeedMapArgs& a, hipStream_t stream)
{
    const dim3 grid((unsigned)a.map.shares), block(256);
    if (a.half_images)
        hipLaunchKernelGGL((seed_importance_kernel<SOURCE, true>), grid, block, 0, stream, a.image0, a.image_ref, a.caller, a.W, a.H,
                           a.map.pixels, a.squared ? 1 : 0, a.floor_q, a.map.q, a.map.chunk_sum);
    else
        hipLaunchKernelGGL((seed_importance_kernel<SOURCE, false>), grid, block, 0, stream, a.image0, a.image_ref, a.caller, a.W, a.H,
                           a.map.pixels, a.squared ? 1 : 0, a.floor_q, a.map.q, a.map.chunk_sum);
}

hipError_t launch_seed_map(const SeedMapArgs& a, hipStream_t stream)
{
    if (a.map.shares == 0) return hipSuccess;
    switch (a.source) {
    case SeedSource::TargetEdges: launch_importance<(int)SeedSource::TargetEdges>(a, stream); break;
    case SeedSource::Error: launch_importance<(int)SeedSource::Error>(a, stream); break;
    case SeedSource::Caller: launch_importance<(int)SeedSource::Caller>(a, stream); break;
    }
    S2D_TRY(hipGetLastError());
    hipLaunchKernelGGL(seed_scan_kernel, dim3(1), dim3(256), 0, stream, (const uint32_t*)a.map.chunk_sum, a.map.shares, a.map.share_prefix);
    return hipGetLastError();
}

hipError_t launch_seed_place(const SeedPlaceArgs& a, hipStream_t stream)
{
    if (a.count <= 0 || a.total == 0 || a.map.shares == 0) return hipSuccess;
    hipLaunchKernelGGL(seed_place_kernel, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

} // namespace s2d
