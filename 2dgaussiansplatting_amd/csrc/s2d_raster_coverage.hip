// s2d_raster_coverage.hip -- the raster kernels of a coverage context (S2D_CFG_COVERAGE) and their dispatch:
// the forward walk that also leaves the pixel's coverage in image0.w, and the backward walk whose channel sum has the coverage as
// a fourth addend.  Both are the shared walks (s2d_walk.h forward_tile, s2d_walk_backward.h backward_tile) with their COVERAGE
// flag set; LDS layout, hand-over, wave sums and flush are those of the plain kernels, and so is the deterministic gather that
// follows a backward walk.
//
// Coverage is the reference's own colour sum (main.cpp:529-531) for a channel whose colour is 1 in every splat, so a plain
// context with the same splats coloured (1, 0, 0) computes it in its red channel operation for operation: that twin is what
// tests/test_gpu_coverage.py holds every bit of the new channel to.
//
// There is no fused kernel, no index-range kernel and no variant with pair counting, the exact exponential or the density
// statistics: the API refuses those combinations, and here they are hipErrorInvalidValue.
#include "s2d_walk_backward.h"

namespace s2d {

template <bool HALF>
__global__ __launch_bounds__(256) void coverage_forward_kernel(const uint32_t* __restrict__ tile_off,
                                                                      const uint32_t* __restrict__ list,
                                                                      const ProjRec* __restrict__ proj, void* __restrict__ image0,
                                                                      unsigned long long* __restrict__ wave_masks,
                                                                      uint32_t* __restrict__ exec_list, uint32_t* __restrict__ tile_exec,
                                                                      uint32_t* __restrict__ retire_hint, Geometry g,
                                                                      const DeviceStatus* __restrict__ status, int abort_stamp,
                                                                      int iteration)
{
    __shared__ FwdShared s;
    if (launch_is_void(status, abort_stamp, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    f2 crg;
    float cb, ca;
    const uint32_t n_exec = forward_tile<false, false, false, true>(s, c, tile_off, list, proj, wave_masks, exec_list, retire_hint, g,
                                                                    nullptr, crg, cb, nullptr, &ca);
    if (c.tid == 0) tile_exec[tile] = n_exec; // the backward walk is another launch
    if (c.inside) store_pixel<HALF>(image0, pixel_index(c, g), make_float4(crg.x, crg.y, cb, ca));
}

// UPSTREAM: image_ref is the caller's dL/d(image0), .w = dL/d(coverage); otherwise the target, whose .w is the alpha to fit
// (tile_sqerr gets the three-channel squared error either way it is formed, main.cpp:796-805).
// (Eight workgroups per CU asked for, as of the fused kernel: left to itself the deterministic variants take 66 VGPRs, one wave
// per SIMD less than the plain kernels; with the bound every variant stays within 64 and none spills -- DESIGN.md section 22.)
template <bool NEED_OP, bool HALF, bool DET, bool UPSTREAM>
__global__ __launch_bounds__(256, 8) void coverage_backward_kernel(const uint32_t* __restrict__ tile_off,
                                                                       const uint32_t* __restrict__ list,
                                                                       const ProjRec* __restrict__ proj,
                                                                       const void* __restrict__ image0,
                                                                       const void* __restrict__ image_ref,
                                                                       const unsigned long long* __restrict__ wave_masks,
                                                                       const uint32_t* __restrict__ exec_list,
                                                                       const uint32_t* __restrict__ tile_exec,
                                                                       float* __restrict__ grads, double* __restrict__ tile_sqerr,
                                                                       Geometry g, DetSlots det,
                                                                       const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ BwdShared<DET> s;
    if (launch_is_void(status, 0, iteration)) return; // the reference abort()ed in an earlier iteration
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    float4 fin = make_float4(0.f, 0.f, 0.f, 0.f), ref = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c.inside) {
        fin = load_pixel<HALF>(image0, pixel_index(c, g)); // finalColor, main.cpp:613, and the final coverage
        ref = load_ref_or_upstream<HALF, UPSTREAM>(image_ref, pixel_index(c, g));
    }
    backward_tile<false, NEED_OP, DET, false, false, UPSTREAM, false, true>(s, c, fin, loss_grad<UPSTREAM, true>(fin, ref), tile_off, list,
                                                                            proj, wave_masks, exec_list, tile_exec[tile], grads,
                                                                            tile_sqerr, g, det, nullptr,
                                                                            SqerrJob{nullptr, 0, nullptr, nullptr});
}

// RasterPass::Forward and RasterPass::Backward of a coverage context (a.coverage).
hipError_t launch_raster_coverage(RasterPass pass, const RasterArgs& a, hipStream_t stream)
{
    const dim3 grid(raster_grid(a.g.num_tiles)), block(256);
    const std::false_type no; // a flag the pass has no variants of
    hipError_t e = hipErrorInvalidValue;
    if (a.count || a.exact_exp || a.density != nullptr) return e;
    switch (pass) {
    case RasterPass::Forward:
        if (a.upstream != nullptr) return e;
        e = with_variant([&](auto, auto, auto half) {
            hipLaunchKernelGGL((coverage_forward_kernel<half>), grid, block, 0, stream, a.tile_off, a.list, a.proj, a.image0,
                               a.wave_masks, a.exec_list, a.tile_exec, a.retire_hint, a.g, a.status, a.abort_stamp, a.iteration);
        }, no, no, a.half_images);
        return e != hipSuccess ? e : hipGetLastError();
    case RasterPass::Backward:
        e = with_variant([&](auto, auto, auto half, auto op, auto d, auto up) {
            hipLaunchKernelGGL((coverage_backward_kernel<op, half, d, up>), grid, block, 0, stream, a.tile_off, a.list, a.proj,
                               a.image0, up ? (const void*)a.upstream : a.image_ref, a.wave_masks, a.exec_list, a.tile_exec, a.grads,
                               up ? nullptr : a.tile_sqerr, a.g, det_slots(a.det), a.status, a.iteration);
        }, no, no, a.half_images, a.need_opacity_grad, a.det.now != 0u, a.upstream != nullptr);
        return e != hipSuccess ? e : launch_det_gather(a, stream);
    default: // no fused launch, no index ranges
        return e;
    }
}

} // namespace s2d
