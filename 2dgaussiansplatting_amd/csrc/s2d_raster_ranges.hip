// s2d_raster_ranges.hip -- the index-range ("chunked") raster kernels and their dispatch: the walks of s2d_walk.h and
// s2d_walk_backward.h over the lists of one index range of the splats at a time, the per-pixel state carried between them.
#include "s2d_walk_backward.h"

namespace s2d {

// ---------------------------------------------------------------------------------------------------
// Index-range ("chunked") rendering, for scenes with more (tile, splat) pairs than one set of lists may hold
// (s2d_sequence.hip chunked_forward / chunked_backward).  The splats are cut into consecutive index ranges; the lists of one range at a time are
// built and walked, front to back like the reference's loops (main.cpp:419, :552), and the per-pixel state is carried
// from range to range in `state` (fp32 whatever the image format): (r, g, b, T).
//   forward pass : raster_forward_chunk_kernel per range; each stores the state and image0 (.w = 1, main.cpp:543-546),
//                  so image0 is final after the last range -- or after the range behind which no pixel is alive any
//                  more (*any_alive stays 0: the host skips the ranges that follow, in both passes).
//   backward pass: raster_backward_chunk_kernel per range, from a fresh state: the forward walk of the range (only for its
//                  hand-over -- the backward walk reads it back, exactly as in the fused kernel) and the backward
//                  walk from the same state, with the FINAL colours of the forward pass out of image0.
// ---------------------------------------------------------------------------------------------------
template <bool HALF, bool EXACT>
__global__ __launch_bounds__(256) void raster_forward_chunk_kernel(const uint32_t* __restrict__ tile_off,
                                                                   const uint32_t* __restrict__ list,
                                                                   const ProjRec* __restrict__ proj, void* __restrict__ image0,
                                                                   float4* __restrict__ state, int first,
                                                                   unsigned long long* __restrict__ wave_masks,
                                                                   uint32_t* __restrict__ exec_list, Geometry g,
                                                                   const DeviceStatus* __restrict__ status, int iteration,
                                                                   uint32_t* __restrict__ any_alive)
{
    __shared__ FwdShared s;
    if (launch_is_void(status, 0, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    float4 st = make_float4(0.0f, 0.0f, 0.0f, 1.0f); // main.cpp:414
    if (!first && c.inside) st = state[pixel_index(c, g)];
    f2 crg = mk2(st.x, st.y);
    float cb = st.z, T = st.w;
    forward_tile<false, EXACT, true>(s, c, tile_off, list, proj, wave_masks, exec_list, nullptr, g, nullptr, crg, cb, &T);
    if (c.inside) {
        state[pixel_index(c, g)] = make_float4(crg.x, crg.y, cb, T);
        store_pixel<HALF>(image0, pixel_index(c, g), make_float4(crg.x, crg.y, cb, 1.0f)); // .w reset, main.cpp:543-546
    }
    if (__ballot(c.inside && !(T < kMinThroughput)) != 0ull && c.lane == 0) atomicOr(any_alive, 1u);
}

template <bool NEED_OP, bool HALF, bool DET, bool EXACT, bool UPSTREAM = false>
__global__ __launch_bounds__(256) void raster_backward_chunk_kernel(const uint32_t* __restrict__ tile_off,
                                                                    const uint32_t* __restrict__ list,
                                                                    const ProjRec* __restrict__ proj,
                                                                    const void* __restrict__ image0,
                                                                    const void* __restrict__ image_ref,
                                                                    float4* __restrict__ state, int first,
                                                                    unsigned long long* __restrict__ wave_masks,
                                                                    uint32_t* __restrict__ exec_list,
                                                                    float* __restrict__ grads, double* __restrict__ tile_sqerr,
                                                                    Geometry g, DetSlots det,
                                                                    const DeviceStatus* __restrict__ status, int iteration)
{
    constexpr size_t kBytes = sizeof(BwdShared<DET>) > sizeof(FwdShared) ? sizeof(BwdShared<DET>) : sizeof(FwdShared);
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
    if (launch_is_void(status, 0, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    float4 st = make_float4(0.0f, 0.0f, 0.0f, 1.0f); // image1 = (0,0,0,1), main.cpp:549
    float4 fin = make_float4(0.f, 0.f, 0.f, 0.f), ref = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c.inside) {
        if (!first) st = state[pixel_index(c, g)];
        fin = load_pixel<HALF>(image0, pixel_index(c, g));    // finalColor, main.cpp:613: of ALL ranges
        ref = load_ref_or_upstream<HALF, UPSTREAM>(image_ref, pixel_index(c, g));
    }
    uint32_t n_exec;
    {   // the executed entries of this range, from the state the backward walk starts from (colours discarded)
        f2 crg = mk2(st.x, st.y);
        float cb = st.z, T = st.w;
        n_exec = forward_tile<false, EXACT, true>(*reinterpret_cast<FwdShared*>(smem), c, tile_off, list, proj, wave_masks, exec_list, nullptr, g,
                                                  nullptr, crg, cb, &T);
    }
    __syncthreads(); // as in the fused kernel: LDS re-use, and the hand-over through global memory
    backward_tile<false, NEED_OP, DET, EXACT, true, UPSTREAM>(*reinterpret_cast<BwdShared<DET>*>(smem), c, fin, loss_grad<UPSTREAM>(fin, ref), tile_off, list, proj,
                                                    wave_masks, exec_list, n_exec, grads, tile_sqerr, g, det, nullptr,
                                                    SqerrJob{nullptr, 0, nullptr, nullptr}, &st);
    if (c.inside) state[pixel_index(c, g)] = st;
}

// ForwardRange and BackwardRange of launch_raster; the backward walk from the target image or from a caller's gradient
// (a.upstream), never with pair counting.
hipError_t launch_raster_ranges(RasterPass pass, const RasterArgs& a, hipStream_t stream)
{
    const dim3 grid(raster_grid(a.g.num_tiles)), block(256);
    const int first = a.first ? 1 : 0;
    const bool det_mode = a.det.now != 0u;
    const std::false_type no; // a flag the pass has no variants of
    const std::true_type yes;
    hipError_t e = hipErrorInvalidValue;
    if (pass == RasterPass::ForwardRange) {
        if (a.upstream != nullptr) return e;
        e = with_variant([&](auto exact, auto, auto half) {
            hipLaunchKernelGGL((raster_forward_chunk_kernel<half, exact>), grid, block, 0, stream, a.tile_off, a.list, a.proj,
                               a.image0, a.state, first, a.wave_masks, a.exec_list, a.g, a.status, a.iteration, a.any_alive);
        }, a.exact_exp, no, a.half_images);
        return e != hipSuccess ? e : hipGetLastError();
    }
    if (pass != RasterPass::BackwardRange) return e;
    if (a.upstream == nullptr)
        e = with_variant([&](auto exact, auto, auto half, auto op, auto d) {
            hipLaunchKernelGGL((raster_backward_chunk_kernel<op, half, d, exact>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, a.image_ref, a.state, first, a.wave_masks, a.exec_list, a.grads, a.tile_sqerr,
                               a.g, det_slots(a.det), a.status, a.iteration);
        }, a.exact_exp, no, a.half_images, a.need_opacity_grad, det_mode);
    else if (!a.count)
        e = with_variant([&](auto exact, auto, auto half, auto op, auto d, auto up) {
            hipLaunchKernelGGL((raster_backward_chunk_kernel<op, half, d, exact, up>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, a.upstream, a.state, first, a.wave_masks, a.exec_list, a.grads, nullptr, a.g,
                               det_slots(a.det), a.status, a.iteration);
        }, a.exact_exp, no, a.half_images, a.need_opacity_grad, det_mode, yes);
    return e != hipSuccess ? e : launch_det_gather(a, stream);
}

} // namespace s2d
