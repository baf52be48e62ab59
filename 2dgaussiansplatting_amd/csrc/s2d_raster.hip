// s2d_raster.hip -- tile-binned forward rasteriser and analytic backward pass.
//
// One 256-thread workgroup (4 wave64) per 16x16 image tile, one thread per pixel.  Each wave owns an 8x8 pixel
// block of the tile, lane = 8 * (row in block) + (column in block).  A tile walks its splat list (ascending splat index ==
// the reference's blend order, main.cpp:419/:552) twice -- forward_tile, then backward_tile -- in batches of 64 entries
// staged in LDS:
//   * forward walk: 4 threads per entry load the 64-byte projected record and evaluate the reference's exact per-row
//     column range (solve_quadratic + int truncation, main.cpp:498-509) for 4 tile rows each, producing one
//     64-bit lane mask per (entry, wave): bit l set <=> the reference's loops visit that pixel for that
//     splat.  The quadratic is solved once per (entry, row), not per pixel.  At the end of a batch the masks and
//     splat indices of the entries whose body ran in at least one wave are stored, compacted to the front of the
//     tile's own range (32 + 4 B per executed pair); the backward walk goes through those entries only, in batches
//     of its own, and loads the masks instead of solving the quadratics again.
//   * after the barrier lane l of every wave fetches the mask of entry l; a ballot of "mask touches a live pixel" is
//     the set of entries this wave has to look at, and the blend loop iterates over its set bits only
//     (scalar bit tricks + v_readlane), skipping an entry with a scalar branch when no lane is live any more.
// A pixel whose throughput fell below 1/256 never works again (main.cpp:520); when all 256 pixels of the tile
// are in that state the workgroup stops walking its list (tile retirement).
//
// Kernels: raster_fused_kernel runs both walks of a tile in one launch, the final colours staying in registers
// (what s2d_step and s2d_forward_backward queue); raster_forward_kernel / raster_backward_kernel run one walk each
// through image0 (s2d_forward / s2d_backward, and the counting diagnostics).
//
// The walks themselves are s2d_walk.h (forward_tile) and s2d_walk_backward.h (backward_tile).  This unit holds the kernels of a
// plain iteration -- forward, backward from the target image, fused, the squared-error sum -- and launch_raster; every other
// kernel family has a unit of its own: s2d_raster_ranges.hip (index ranges), s2d_raster_gradient.hip
// (backward from a caller's gradient, density statistics), s2d_raster_det.hip (deterministic mode's gather),
// s2d_raster_reference.hip (reference-order validation), s2d_raster_coverage.hip (the coverage channel), s2d_backdrop.hip (the
// forward walk over a backdrop).
//
// The alpha / throughput / colour arithmetic is the reference's, operation for operation
// (-ffp-contract=off), in both walks, so the framebuffer is bit-identical to the oracle's and the backward
// walk makes exactly the forward's per-pixel decisions.  The backward walk then sums each splat's nine
// partial gradients over the wave through an LDS transpose (wave_sum8_lds), over the four waves in one LDS slot per
// entry, and issues one global float-atomic burst per (tile, splat) into the N x 9 gradient array -- or,
// with S2D_CFG_DETERMINISTIC, keeps one slot per wave, adds them in a fixed order and stores the partial into the
// tile's own slot of that splat, and a gather kernel sums each splat's slots in a fixed order (bitwise
// reproducible gradients).
#include "s2d_backdrop.h"
#include "s2d_walk_backward.h"

namespace s2d {

template <bool COUNT, bool HALF, bool EXACT>
__global__ __launch_bounds__(256) void raster_forward_kernel(const uint32_t* __restrict__ tile_off,
                                                             const uint32_t* __restrict__ list,
                                                             const ProjRec* __restrict__ proj,
                                                             void* __restrict__ image0,
                                                             unsigned long long* __restrict__ wave_masks,
                                                             uint32_t* __restrict__ exec_list, uint32_t* __restrict__ tile_exec,
                                                             uint32_t* __restrict__ retire_hint,
                                                             Geometry g, const DeviceStatus* __restrict__ status, int abort_stamp,
                                                             int iteration, PairCounters* __restrict__ counters)
{
    __shared__ FwdShared s;
    if (launch_is_void(status, abort_stamp, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    f2 crg;
    float cb;
    const uint32_t n_exec = forward_tile<COUNT, EXACT>(s, c, tile_off, list, proj, wave_masks, exec_list, retire_hint, g, counters, crg, cb);
    if (!COUNT && c.tid == 0) tile_exec[tile] = n_exec; // the backward walk is another launch
    if (c.inside) store_pixel<HALF>(image0, pixel_index(c, g), make_float4(crg.x, crg.y, cb, 1.0f)); // .w reset, main.cpp:543-546
}

// Forward and backward walk of a tile in ONE launch (what s2d_step and s2d_forward_backward queue): a tile's backward
// pass needs nothing but its own pixels' final colours, which are still in registers when the forward walk ends.  One
// dispatch, one ramp-down tail and one read of image0 (16 B per pixel) less per iteration than the two kernels above,
// which remain for callers that run the passes separately.  The executed entries still travel through exec_list and
// wave_masks: written by the entry's staging threads and read back by other threads of the same workgroup (so they rarely
// leave L2); the __syncthreads() between the walks orders the two at workgroup scope, and their number stays in a
// register (tile_exec is written for an s2d_backward that may follow).  With S2D_CFG_FP16_IMAGES the backward walk sees the
// final colour as stored, i.e. rounded to fp16, exactly like the separate kernels.  image0 is written only when
// `write_image` is set (s2d_step: the last iteration of the call; nothing else reads it).
template <bool NEED_OP, bool HALF, bool DET, bool EXACT>
__global__ __launch_bounds__(256, 8) void raster_fused_kernel(const uint32_t* __restrict__ tile_off,
                                                           const uint32_t* __restrict__ list,
                                                           const ProjRec* __restrict__ proj, void* __restrict__ image0,
                                                           const void* __restrict__ image_ref,
                                                           unsigned long long* __restrict__ wave_masks,
                                                           uint32_t* __restrict__ exec_list, uint32_t* __restrict__ tile_exec,
                                                           uint32_t* __restrict__ retire_hint,
                                                           float* __restrict__ grads, double* __restrict__ tile_sqerr,
                                                           Geometry g, DetSlots det,
                                                           const DeviceStatus* __restrict__ status, int abort_stamp,
                                                           int iteration, int write_image, SqerrJob sq)
{
    constexpr size_t kBytes = sizeof(BwdShared<DET>) > sizeof(FwdShared) ? sizeof(BwdShared<DET>) : sizeof(FwdShared);
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes]; // the two walks use the same LDS one after the other
    if (launch_is_void(status, abort_stamp, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    f2 crg;
    float cb;
    const uint32_t n_exec = forward_tile<false, EXACT>(*reinterpret_cast<FwdShared*>(smem), c, tile_off, list, proj, wave_masks,
                                                       exec_list, retire_hint, g, nullptr, crg, cb);
    if (c.tid == 0) tile_exec[tile] = n_exec;
    float4 fin = make_float4(crg.x, crg.y, cb, 1.0f), ref = make_float4(0.f, 0.f, 0.f, 0.f);
    if (HALF) { // what the backward pass would read back from the fp16 framebuffer
        const __half2 a = __floats2half2_rn(fin.x, fin.y), b = __floats2half2_rn(fin.z, fin.w);
        const float2 fa = __half22float2(a), fb = __half22float2(b);
        fin = make_float4(fa.x, fa.y, fb.x, fb.y);
    }
    if (c.inside) {
        if (write_image) store_pixel<HALF>(image0, pixel_index(c, g), fin); // .w reset, main.cpp:543-546
        ref = load_pixel<HALF>(image_ref, pixel_index(c, g));
    } else {
        fin = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the backward walk re-uses the LDS the forward walk's hand-over may still be reading, and reads what other threads
    // of the workgroup handed over through global memory
    __syncthreads();
    backward_tile<false, NEED_OP, DET, EXACT>(*reinterpret_cast<BwdShared<DET>*>(smem), c, fin, loss_grad<false>(fin, ref), tile_off,
                                              list, proj, wave_masks, exec_list, n_exec, grads, tile_sqerr, g, det, nullptr, sq);
}

// Sum of the per-tile squared errors in a fixed order (deterministic MSE trace), two stages in one launch:
// kSqerrChunks blocks each reduce a contiguous chunk to partial[b] (sqerr_reduce, s2d_device.h); the block that finishes last (ticket counter)
// adds the partials, again in a fixed order, and re-arms the counter.  scratch = kSqerrChunks doubles + one
// 64-bit counter, zero before the first launch (SqerrTrace, s2d_state.hip, allocates it behind tile_sqerr).
__global__ __launch_bounds__(256) void sqerr_finalize_kernel(const double* __restrict__ tile_sqerr, int num_tiles,
                                                             double* __restrict__ out, double* scratch,
                                                             const DeviceStatus* __restrict__ status, int iteration)
{
    if (status->first_nonfinite_iter < iteration) return;
    sqerr_reduce(tile_sqerr, num_tiles, out, scratch, (int)blockIdx.x, kSqerrChunks);
}

// Which unit's kernels run a pass: the pass, then whether the backward walk starts from the target image or from a caller's
// gradient (a.upstream), then whether it also sums the density statistics (a.density).  Only the backward kernels have the last
// two; a combination without a kernel is hipErrorInvalidValue.  A coverage context (a.coverage) has its own forward and backward
// kernels and no others.  A backdrop (a.backdrop, s2d_backdrop.hip) has a forward kernel of its own; its backward walks are the
// plain ones, and it has no fused launch and no index ranges.
hipError_t launch_raster(RasterPass pass, const RasterArgs& a, hipStream_t stream)
{
    if (a.g.num_tiles <= 0) return hipSuccess;
    if (a.coverage) return launch_raster_coverage(pass, a, stream);
    if (a.backdrop != nullptr && pass != RasterPass::Backward)
        return pass == RasterPass::Forward ? launch_raster_backdrop(a, stream) : hipErrorInvalidValue;
    const dim3 grid(raster_grid(a.g.num_tiles)), block(256);
    const bool from_target = a.upstream == nullptr, stats = a.density != nullptr;
    const bool det_mode = a.det.now != 0u;
    const std::false_type no; // a flag the pass has no variants of
    hipError_t e = hipErrorInvalidValue;
    switch (pass) {
    case RasterPass::Forward:
        if (!from_target || stats) return e;
        e = with_variant([&](auto exact, auto count, auto half) {
            hipLaunchKernelGGL((raster_forward_kernel<count, half, exact>), grid, block, 0, stream, a.tile_off, a.list, a.proj,
                               a.image0, a.wave_masks, a.exec_list, a.tile_exec, a.retire_hint, a.g, a.status, a.abort_stamp,
                               a.iteration, a.counters);
        }, a.exact_exp, a.count, a.half_images);
        return e != hipSuccess ? e : hipGetLastError();
    case RasterPass::Fused: // (pair counting is a property of the separate kernels)
        if (!from_target || stats) return e;
        e = with_variant([&](auto exact, auto, auto half, auto op, auto d) {
            hipLaunchKernelGGL((raster_fused_kernel<op, half, d, exact>), grid, block, 0, stream, a.tile_off, a.list, a.proj,
                               a.image0, a.image_ref, a.wave_masks, a.exec_list, a.tile_exec, a.retire_hint, a.grads, a.tile_sqerr,
                               a.g, det_slots(a.det), a.status, a.abort_stamp, a.iteration, a.write_image ? 1 : 0, a.sq);
        }, a.exact_exp, no, a.half_images, a.need_opacity_grad, det_mode);
        break;
    case RasterPass::Backward:
        if (!from_target || stats) return launch_raster_gradient(a, stream);
        e = with_variant([&](auto exact, auto count, auto half, auto op, auto d) {
            hipLaunchKernelGGL((raster_backward_kernel<count, op, half, d, exact>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, a.image_ref, a.wave_masks, a.exec_list, a.tile_exec, a.grads, a.tile_sqerr, a.g,
                               det_slots(a.det), a.status, a.iteration, a.counters);
        }, a.exact_exp, a.count, a.half_images, a.need_opacity_grad, det_mode);
        break;
    case RasterPass::ForwardRange:
    case RasterPass::BackwardRange:
        return stats ? e : launch_raster_ranges(pass, a, stream);
    }
    return e != hipSuccess ? e : launch_det_gather(a, stream);
}

hipError_t launch_sqerr_finalize(SqerrJob sq, const DeviceStatus* status, int iteration, hipStream_t stream)
{
    hipLaunchKernelGGL(sqerr_finalize_kernel, dim3(kSqerrChunks), dim3(256), 0, stream, sq.tile_sqerr, sq.num_tiles, sq.out,
                       sq.scratch, status, iteration);
    return hipGetLastError();
}

} // namespace s2d
