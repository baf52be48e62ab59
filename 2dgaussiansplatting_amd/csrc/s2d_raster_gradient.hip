// s2d_raster_gradient.hip -- the instantiations of raster_backward_kernel (s2d_walk_backward.h) that start from a caller's loss
// gradient (UPSTREAM: a.upstream in the place of image_ref) or also sum the density statistics (STATS),
// and their dispatch.
#include "s2d_walk_backward.h"

namespace s2d {

// RasterPass::Backward with a.upstream or a.density: never with pair counting, and the statistics not with the exact
// exponential either.
hipError_t launch_raster_gradient(const RasterArgs& a, hipStream_t stream)
{
    const dim3 grid(raster_grid(a.g.num_tiles)), block(256);
    const bool det_mode = a.det.now != 0u;
    const std::false_type no; // a flag the pass has no variants of
    const std::true_type yes;
    hipError_t e = hipErrorInvalidValue;
    if (a.count) return e;
    if (a.density == nullptr)
        e = with_variant([&](auto exact, auto, auto half, auto op, auto d, auto up) {
            hipLaunchKernelGGL((raster_backward_kernel<false, op, half, d, exact, up>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, a.upstream, a.wave_masks, a.exec_list, a.tile_exec, a.grads, nullptr, a.g,
                               det_slots(a.det), a.status, a.iteration, nullptr);
        }, a.exact_exp, no, a.half_images, a.need_opacity_grad, det_mode, yes);
    else if (!a.exact_exp)
        e = with_variant([&](auto, auto, auto half, auto op, auto d, auto up, auto st) {
            hipLaunchKernelGGL((raster_backward_kernel<false, op, half, d, false, up, st>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, up ? (const void*)a.upstream : a.image_ref, a.wave_masks, a.exec_list, a.tile_exec,
                               a.grads, up ? nullptr : a.tile_sqerr, a.g, det_slots(a.det), a.status, a.iteration, nullptr,
                               a.density);
        }, no, no, a.half_images, a.need_opacity_grad, det_mode, a.upstream != nullptr, yes);
    return e != hipSuccess ? e : launch_det_gather(a, stream);
}

} // namespace s2d
