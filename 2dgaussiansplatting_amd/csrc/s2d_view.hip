// s2d_view.hip -- view rendering: the record transform and the view raster kernel (s2d_view.h).
//
// view_raster_kernel is two pieces of s2d_view_walk.h, one after the other: the sample walk of the tile (view_walk_tile: the
// forward walk over the lists of the view's raster grid without anything that serves training, 5.1 KB of LDS) and the resolve
// of S x S samples to an output pixel with its store (view_resolve_store: lane exchange, RGBA32F or RGBA8).  One 256-thread
// workgroup per 16 x 16 tile of the grid, four wave64 of 8 x 8 samples, lane = 8 * row + column.  backdrop_view_kernel
// (s2d_backdrop.hip) is the same two pieces with the composite between them.
//
// COVERAGE (S2D_CFG_COVERAGE): the walk blends through blend_entry_coverage, the coverage goes through the
// same resolve as the colours and ends in .w (RGBA8: the alpha byte, quantised like the colours).
#include "s2d_view_walk.h"

namespace s2d {

__global__ __launch_bounds__(256) void view_transform_kernel(const float* __restrict__ splats, int n, ViewXform x,
                                                             float* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float in9[9], out9[9];
#pragma unroll
    for (int k = 0; k < 9; k++) in9[k] = splats[(size_t)i * 9 + k];
    view_row(x, in9, out9);
#pragma unroll
    for (int k = 0; k < 9; k++) out[(size_t)i * 9 + k] = out9[k];
}

template <bool EXACT, int S, bool RGBA8, bool COVERAGE = false>
__global__ __launch_bounds__(256) void view_raster_kernel(const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ list,
                                                          const ProjRec* __restrict__ proj, void* __restrict__ out, Geometry g,
                                                          int out_width)
{
    __shared__ ViewShared s;
    const int tile = (int)blockIdx.x;
    if (tile >= g.num_tiles) return;
    view_resolve_store<S, RGBA8, COVERAGE>(view_walk_tile<EXACT, COVERAGE>(s, tile, tile_off, list, proj, g), out, out_width);
}

hipError_t launch_view_transform(const float* splats, int n, ViewXform x, float* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(view_transform_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, splats, n, x, out);
    return hipGetLastError();
}

hipError_t launch_view_raster(const ViewRasterArgs& a, hipStream_t stream)
{
    const RasterArgs& w = a.walk;
    if (w.g.num_tiles <= 0) return hipErrorInvalidValue;
    if (w.coverage && w.exact_exp) return hipErrorInvalidValue; // a missing kernel is an error (the coverage kernels exist with exp_approx alone)
    const dim3 grid((unsigned)w.g.num_tiles), block(256);
    const std::false_type no; // flags the view has no variants of: pair counting, fp16 images
    const hipError_t e = with_samples(a.samples, [&](auto samples) {
        constexpr int S = decltype(samples)::value;
        return with_variant([&](auto exact, auto, auto, auto rgba8, auto coverage) {
            if constexpr (!(exact && coverage))
                hipLaunchKernelGGL((view_raster_kernel<exact, S, rgba8, coverage>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.out,
                                   w.g, a.out_width);
        }, w.exact_exp, no, no, a.rgba8, w.coverage);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

} // namespace s2d
