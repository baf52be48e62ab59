// s2d_view_gradient.hip -- the backward pass through a view (s2d_view.h): view_gradient_kernel, which
// turns dL/d(view) into the gradients of the view's records, and view_adjoint_kernel, which takes those back through the record
// transform (s2d_view_math.h view_row_adjoint) and adds them into the context's gradient buffer.
//
// view_gradient_kernel is composed from the shared walks the way raster_fused_kernel (s2d_raster.hip) is: forward_tile over the
// view's lists leaves the final colour of every sample in registers and hands the executed entries over; backward_tile
// (UPSTREAM: the loss is the caller's, no squared error) walks them from those registers.  One 256-thread workgroup per 16 x 16
// tile of the raster grid (out * S), four wave64 of 8 x 8 samples, lane = 8 * row + column.  The hand-over and the retirement
// hint are buffers of the view (ViewScratch), never the context's, so a training pass in flight keeps what it handed over.
//
// Between the walks stands the adjoint of the resolve, in lanes, made of the pieces of s2d_view_walk.h that view_fit_kernel
// (s2d_view_fit.hip) is made of too.  An S x S block of samples lies inside one wave's 8 x 8 block and its top-left lane is the
// one view_raster_kernel stores the output pixel from (view_top_lane).  Here that lane loads the pixel's upstream gradient (one
// float4), every lane of the block reads it from there and multiplies it by 0.25f once per level of the resolve
// (view_broadcast) -- exact, so a NumPy `repeat` times 0.25^levels gives the same bits.  No supersampled image or gradient image
// exists in memory.  FROM_TARGET: the buffer holds a target of the view's size instead; the forward resolve is
// view_raster_kernel's (view_resolve), the top-left lane forms resolved - target, one fp32 subtraction per channel
// (view_minus_target), and the broadcast is the same.  Samples outside the grid enter the backward walk with zeros
// (view_zero_outside).
//
// LDS: the two walks use the same bytes one after the other, max(sizeof(FwdShared), sizeof(BwdShared<DET>)) as in the fused
// kernel -- 19.3 KB (17.5 KB deterministic), the same eight workgroups per CU (__launch_bounds__(256, 8): 64 VGPRs).  The one
// exception is the exact exponential in deterministic mode, a validation mode twice over: under the 64-register bound it spills
// three dwords per lane (as the fused kernel's variant does), so those instantiations are bound to four workgroups instead
// and keep everything in registers (66 VGPRs: seven workgroups per CU) -- no variant of this unit uses scratch.
#include "s2d_view_walk.h"
#include "s2d_walk_backward.h"

namespace s2d {

template <bool EXACT, int S, bool NEED_OP, bool DET, bool FROM_TARGET>
__global__ __launch_bounds__(256, (EXACT && DET) ? 4 : 8) void view_gradient_kernel(const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ list,
                                                               const ProjRec* __restrict__ proj, const float4* __restrict__ src,
                                                               unsigned long long* __restrict__ wave_masks,
                                                               uint32_t* __restrict__ exec_list, uint32_t* __restrict__ tile_exec,
                                                               uint32_t* __restrict__ retire_hint, float* __restrict__ grads,
                                                               Geometry g, int out_width, DetSlots det)
{
    static_assert(S == 1 || S == 2 || S == 4, "samples per axis");
    constexpr size_t kBytes = sizeof(BwdShared<DET>) > sizeof(FwdShared) ? sizeof(BwdShared<DET>) : sizeof(FwdShared);
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes]; // the two walks use the same LDS one after the other
    const int tile = (int)blockIdx.x;
    if (tile >= g.num_tiles) return;
    const TileCtx c = tile_ctx(tile, g);
    f2 crg;
    float cb;
    const uint32_t n_exec = forward_tile<false, EXACT>(*reinterpret_cast<FwdShared*>(smem), c, tile_off, list, proj, wave_masks,
                                                       exec_list, retire_hint, g, nullptr, crg, cb);
    if (c.tid == 0) tile_exec[tile] = n_exec;
    float4 fin = make_float4(crg.x, crg.y, cb, 1.0f);

    size_t o;
    const bool top = view_top_lane<S>(c, out_width, &o);
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
    if (FROM_TARGET) u = view_minus_target<S>(fin, top, src, o);
    else if (top) u = src[o];
    view_broadcast<S>(u, c.lane);
    view_zero_outside(c, fin, u);
    // the backward walk re-uses the LDS the forward walk's hand-over may still be reading, and reads what other threads
    // of the workgroup handed over through global memory
    __syncthreads();
    backward_tile<false, NEED_OP, DET, EXACT, false, true>(*reinterpret_cast<BwdShared<DET>*>(smem), c, fin, u, tile_off, list, proj,
                                                           wave_masks, exec_list, n_exec, grads, nullptr, g, det, nullptr,
                                                           SqerrJob{nullptr, 0, nullptr, nullptr});
}

// grads[i] += view_row_adjoint(x, splats[i], view_grads[i]) for the rows of the capacity; a row that is not alive (held[i] == 0)
// has no footprint in the view and is left as it is.
__global__ __launch_bounds__(256) void view_adjoint_kernel(const float* __restrict__ splats, const uint8_t* __restrict__ held, int n,
                                                           ViewXform x, const float* __restrict__ view_grads, float* __restrict__ grads)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (held != nullptr && held[i] == 0) return;
    float in9[9], gv[9], go[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        in9[k] = splats[(size_t)i * 9 + k];
        gv[k] = view_grads[(size_t)i * 9 + k];
    }
    view_row_adjoint(x, in9, gv, go);
#pragma unroll
    for (int k = 0; k < 9; k++) grads[(size_t)i * 9 + k] += go[k];
}

hipError_t launch_view_gradient(const ViewGradientArgs& a, hipStream_t stream)
{
    const RasterArgs& w = a.walk;
    if (w.g.num_tiles <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)w.g.num_tiles), block(256);
    const std::false_type no; // flags the view has no variants of: pair counting, fp16 images
    const hipError_t e = with_samples(a.samples, [&](auto samples) {
        constexpr int S = decltype(samples)::value;
        return with_variant([&](auto exact, auto, auto, auto op, auto d, auto ft) {
            hipLaunchKernelGGL((view_gradient_kernel<exact, S, op, d, ft>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.src,
                               w.wave_masks, w.exec_list, w.tile_exec, w.retire_hint, w.grads, w.g, a.out_width, det_slots(w.det));
        }, w.exact_exp, no, no, w.need_opacity_grad, w.det.now != 0u, a.from_target);
    });
    if (e != hipSuccess) return e;
    return launch_det_gather(w, stream); // deterministic mode: the slots of the view's rectangles, summed in slot order into walk.grads
}

hipError_t launch_view_adjoint(const float* splats, const uint8_t* held, int n, ViewXform x, const float* view_grads, float* grads,
                               hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(view_adjoint_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, splats, held, n, x, view_grads, grads);
    return hipGetLastError();
}

} // namespace s2d
