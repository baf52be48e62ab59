// s2d_backdrop.hip -- the kernels of a backdrop (include/splat2d_backdrop.h, s2d_backdrop.h) and their
// launches: the forward walk that composites over the backdrop and leaves T_final, the view over a constant backdrop (the sample
// walk and the resolve of s2d_view_walk.h with the composite between them), and the gradient of the backdrop.
//
// image0.c = C.c + (T_final * B.c), one fp32 multiply and one add (-ffp-contract=off).  The reference's loop throws T_final away
// (main.cpp:543-546); forward_tile (s2d_walk.h) has it in a register when the walk ends and, with its THROUGHPUT flag, hands it
// back: the plain walk -- the reference's operations in the reference's order, the hand-over to the backward walk, the
// retirement hint -- and nothing else.  (The walk of the index ranges, CHUNK, hands T back too and would have needed no flag,
// but it sizes its batches without the hint: measured 8.7 to 9.2 % slower than raster_forward_kernel at 4096^2 / 1 M, against
// -1.1 to +0.9 % for this one)
//
// Nothing else of an iteration is here.  The backward kernels read the final colour from image0 and form S = fin - running
// (main.cpp:627): with the composite stored, S carries the backdrop's share, and c * T - S / (1 - alpha) (main.cpp:628) is the
// derivative of the composite with respect to alpha.  Both walks skip the same splats below the throughput cut-off
// (main.cpp:520), so this holds across it.
//
// There is no variant with pair counting, the exact exponential, the coverage channel or index ranges: the API refuses those
// combinations (s2d_api_backdrop.hip), and a pass without a kernel is hipErrorInvalidValue.
#include "s2d_backdrop.h"
#include "s2d_view_walk.h"
#include "s2d_walk_backward.h"

namespace s2d {

struct BackdropRgb { // a constant backdrop as a kernel argument
    float r, g, b;
};

// PLANE: the backdrop of a pixel is plane[pixel].xyz instead of `constant`.
template <bool HALF, bool PLANE>
__global__ __launch_bounds__(256) void backdrop_forward_kernel(const uint32_t* __restrict__ tile_off,
                                                                const uint32_t* __restrict__ list,
                                                                const ProjRec* __restrict__ proj, void* __restrict__ image0,
                                                                unsigned long long* __restrict__ wave_masks,
                                                                uint32_t* __restrict__ exec_list, uint32_t* __restrict__ tile_exec,
                                                                Geometry g, const DeviceStatus* __restrict__ status, int abort_stamp,
                                                                int iteration, BackdropRgb constant, const float4* __restrict__ plane,
                                                                float* __restrict__ throughput, uint32_t* __restrict__ retire_hint)
{
    __shared__ FwdShared s;
    if (launch_is_void(status, abort_stamp, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    f2 crg;
    float cb, T;
    const uint32_t n_exec = forward_tile<false, false, false, false, true>(s, c, tile_off, list, proj, wave_masks, exec_list, retire_hint,
                                                                           g, nullptr, crg, cb, &T);
    if (c.tid == 0) tile_exec[tile] = n_exec; // the backward walk is another launch
    if (c.inside) {
        const size_t i = pixel_index(c, g);
        BackdropRgb b = constant;
        if (PLANE) {
            const float4 p = plane[i];
            b = BackdropRgb{p.x, p.y, p.z};
        }
        store_pixel<HALF>(image0, i, make_float4(crg.x + (T * b.r), crg.y + (T * b.g), cb + (T * b.b), 1.0f)); // .w reset, main.cpp:543-546
        throughput[i] = T;
    }
}

// view_raster_kernel<false, S, RGBA8> (s2d_view.hip) with the composite per sample: the same sample walk (s2d_view_walk.h), then
// c += T * B, one fp32 multiply and one add per channel, then the same resolve and store.
template <int S, bool RGBA8>
__global__ __launch_bounds__(256) void backdrop_view_kernel(const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ list,
                                                            const ProjRec* __restrict__ proj, void* __restrict__ out, Geometry g,
                                                            int out_width, BackdropRgb constant)
{
    __shared__ ViewShared s;
    const int tile = (int)blockIdx.x;
    if (tile >= g.num_tiles) return;
    ViewSample p = view_walk_tile<false, false>(s, tile, tile_off, list, proj, g);
    p.cr = p.cr + (p.T * constant.r); // the composite of the sample
    p.cg = p.cg + (p.T * constant.g);
    p.cb = p.cb + (p.T * constant.b);
    view_resolve_store<S, RGBA8, false>(p, out, out_width);
}

// t_c = T_final * g_c per pixel and channel (one fp32 multiply), g = upstream or image0 - image_ref (loss_grad).  Workgroup b of
// the grid takes pixels b * 256 + thread, + grid * 256, ...: each thread adds its terms in double in that order, the workgroup
// adds its threads' sums (block_sum_256: a fixed tree) and stores three partials.  partials == nullptr: the terms alone.
template <bool HALF, bool UPSTREAM>
__global__ __launch_bounds__(256) void backdrop_grad_kernel(const float* __restrict__ throughput, const void* __restrict__ image0,
                                                            const void* __restrict__ image_ref, const float4* __restrict__ upstream,
                                                            size_t pixels, float4* __restrict__ dplane, double* __restrict__ partials)
{
    __shared__ double s4[4];
    double ar = 0.0, ag = 0.0, ab = 0.0;
    const size_t stride = (size_t)gridDim.x * 256u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < pixels; i += stride) {
        float4 gr;
        if (UPSTREAM) gr = upstream[i];
        else gr = loss_grad<false>(load_pixel<HALF>(image0, i), load_pixel<HALF>(image_ref, i));
        const float t = throughput[i];
        const float tr = t * gr.x, tg = t * gr.y, tb = t * gr.z;
        if (dplane != nullptr) dplane[i] = make_float4(tr, tg, tb, 0.0f);
        ar += (double)tr;
        ag += (double)tg;
        ab += (double)tb;
    }
    if (partials == nullptr) return; // (uniform)
    const double r = block_sum_256(ar, s4), gsum = block_sum_256(ag, s4), b = block_sum_256(ab, s4);
    if (threadIdx.x == 0) {
        partials[(size_t)blockIdx.x * 3 + 0] = r;
        partials[(size_t)blockIdx.x * 3 + 1] = gsum;
        partials[(size_t)blockIdx.x * 3 + 2] = b;
    }
}

// The fixed-order finish: one workgroup, thread t holds the partials of workgroup t (blocks <= 256), the same tree again.
__global__ __launch_bounds__(256) void backdrop_grad_finish_kernel(const double* __restrict__ partials, int blocks, double* __restrict__ sums)
{
    __shared__ double s4[4];
    const bool have = (int)threadIdx.x < blocks;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double v = block_sum_256(have ? partials[(size_t)threadIdx.x * 3 + k] : 0.0, s4);
        if (threadIdx.x == 0) sums[k] = v;
    }
}

// RasterPass::Forward of a context with a backdrop (a.backdrop).
hipError_t launch_raster_backdrop(const RasterArgs& a, hipStream_t stream)
{
    const BackdropArgs* b = a.backdrop;
    if (b == nullptr || b->throughput == nullptr) return hipErrorInvalidValue;
    if (a.count || a.exact_exp || a.coverage || a.upstream != nullptr || a.density != nullptr) return hipErrorInvalidValue; // a missing kernel is an error
    const dim3 grid(raster_grid(a.g.num_tiles)), block(256);
    const std::false_type no; // a flag the pass has no variants of
    const BackdropRgb constant{b->rgb[0], b->rgb[1], b->rgb[2]};
    const hipError_t e = with_variant([&](auto, auto, auto half, auto plane) {
        hipLaunchKernelGGL((backdrop_forward_kernel<half, plane>), grid, block, 0, stream, a.tile_off, a.list, a.proj, a.image0,
                           a.wave_masks, a.exec_list, a.tile_exec, a.g, a.status, a.abort_stamp, a.iteration, constant, b->plane,
                           b->throughput, a.retire_hint);
    }, no, no, a.half_images, b->plane != nullptr);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_backdrop_view(const ViewRasterArgs& a, hipStream_t stream)
{
    const RasterArgs& w = a.walk;
    if (w.g.num_tiles <= 0 || w.exact_exp || w.coverage) return hipErrorInvalidValue; // a missing kernel is an error
    const dim3 grid((unsigned)w.g.num_tiles), block(256);
    const BackdropRgb constant{a.rgb[0], a.rgb[1], a.rgb[2]};
    const hipError_t e = with_samples(a.samples, [&](auto samples) {
        constexpr int S = decltype(samples)::value;
        if (a.rgba8)
            hipLaunchKernelGGL((backdrop_view_kernel<S, true>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.out, w.g, a.out_width, constant);
        else
            hipLaunchKernelGGL((backdrop_view_kernel<S, false>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.out, w.g, a.out_width, constant);
        return hipSuccess;
    });
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_backdrop_grads(const BackdropGradArgs& a, hipStream_t stream)
{
    if (a.throughput == nullptr || a.pixels == 0 || (a.partials != nullptr) != (a.sums != nullptr)) return hipErrorInvalidValue;
    if (a.upstream == nullptr && (a.image0 == nullptr || a.image_ref == nullptr)) return hipErrorInvalidValue;
    const int blocks = (int)std::min<size_t>((a.pixels + 255) / 256, (size_t)kBackdropGradBlocks);
    const dim3 grid((unsigned)blocks), block(256);
    if (a.upstream != nullptr)
        hipLaunchKernelGGL((backdrop_grad_kernel<false, true>), grid, block, 0, stream, a.throughput, a.image0, a.image_ref, a.upstream,
                           a.pixels, a.dplane, a.partials);
    else if (a.half_images)
        hipLaunchKernelGGL((backdrop_grad_kernel<true, false>), grid, block, 0, stream, a.throughput, a.image0, a.image_ref, a.upstream,
                           a.pixels, a.dplane, a.partials);
    else
        hipLaunchKernelGGL((backdrop_grad_kernel<false, false>), grid, block, 0, stream, a.throughput, a.image0, a.image_ref, a.upstream,
                           a.pixels, a.dplane, a.partials);
    S2D_TRY(hipGetLastError());
    if (a.partials == nullptr) return hipSuccess;
    hipLaunchKernelGGL(backdrop_grad_finish_kernel, dim3(1), block, 0, stream, a.partials, blocks, a.sums);
    return hipGetLastError();
}

} // namespace s2d
