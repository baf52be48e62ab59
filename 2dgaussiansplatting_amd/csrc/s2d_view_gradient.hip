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
// Between the walks stands the adjoint of the resolve, in lanes.  An S x S block of samples lies inside one wave's 8 x 8 block
// and its top-left lane is the one view_raster_kernel stores the output pixel from.  Here that lane loads the pixel's upstream
// gradient (one float4), every lane of the block reads it from there (__shfl from lane & ~mask, mask = the lane bits of the
// block: 1 | 8, and for S = 4 also 2 | 16) and multiplies it by 0.25f once per level of the resolve -- exact, so a NumPy
// `repeat` times 0.25^levels gives the same bits.  No supersampled image or gradient image exists in memory.  FROM_TARGET: the
// buffer holds a target of the view's size instead; the forward resolve runs as in view_raster_kernel (resolve_level), the
// top-left lane forms resolved - target, one fp32 subtraction per channel, and the broadcast is the same.
//
// LDS: the two walks use the same bytes one after the other, max(sizeof(FwdShared), sizeof(BwdShared<DET>)) as in the fused
// kernel -- 19.3 KB (17.5 KB deterministic), the same eight workgroups per CU (__launch_bounds__(256, 8): 64 VGPRs).  The one
// exception is the exact exponential in deterministic mode, a validation mode twice over: under the 64-register bound it spills
// three dwords per lane (as the fused kernel's variant does), so those instantiations are bound to four workgroups instead
// and keep everything in registers (66 VGPRs: seven workgroups per CU) -- no variant of this unit uses scratch.
#include "s2d_view.h"
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

    // the top-left sample of an output pixel (S divides 8, so the block is inside the grid as a whole or not at all)
    int lx, ly;
    pixel_of_thread(c.tid, &lx, &ly);
    const bool top = c.inside && (lx % S) == 0 && (ly % S) == 0;
    const size_t o = (size_t)(c.y / S) * (size_t)out_width + (size_t)(c.x / S);
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
    if (FROM_TARGET) {
        float rr = fin.x, rg = fin.y, rb = fin.z; // the view's pixel, as view_raster_kernel resolves it
        if (S >= 2) {
            rr = resolve_level<1, 8>(rr);
            rg = resolve_level<1, 8>(rg);
            rb = resolve_level<1, 8>(rb);
        }
        if (S == 4) {
            rr = resolve_level<2, 16>(rr);
            rg = resolve_level<2, 16>(rg);
            rb = resolve_level<2, 16>(rb);
        }
        if (top) {
            const float4 t = src[o];
            u = make_float4(rr - t.x, rg - t.y, rb - t.z, 0.0f);
        }
    } else if (top) {
        u = src[o];
    }
    if (S >= 2) {
        constexpr int kBlockBits = S == 4 ? (1 | 2 | 8 | 16) : (1 | 8);
        constexpr int kLevels = S == 4 ? 2 : 1;
        const int from = c.lane & ~kBlockBits;
        u.x = __shfl(u.x, from, 64);
        u.y = __shfl(u.y, from, 64);
        u.z = __shfl(u.z, from, 64);
#pragma unroll
        for (int l = 0; l < kLevels; l++) {
            u.x *= 0.25f;
            u.y *= 0.25f;
            u.z *= 0.25f;
        }
    }
    if (!c.inside) {
        fin = make_float4(0.f, 0.f, 0.f, 0.f);
        u = make_float4(0.f, 0.f, 0.f, 0.f);
    }
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

namespace {

template <bool EXACT, int S>
hipError_t launch_view_gradient_flags(const ViewGradientArgs& a, hipStream_t stream)
{
    const RasterArgs& w = a.walk;
    const dim3 grid((unsigned)w.g.num_tiles), block(256);
    const std::false_type no; // flags the view has no variants of: pair counting, fp16 images
    return with_variant([&](auto, auto, auto, auto op, auto d, auto ft) {
        hipLaunchKernelGGL((view_gradient_kernel<EXACT, S, op, d, ft>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.src,
                           w.wave_masks, w.exec_list, w.tile_exec, w.retire_hint, w.grads, w.g, a.out_width, det_slots(w.det));
    }, std::bool_constant<EXACT>{}, no, no, w.need_opacity_grad, w.det.now != 0u, a.from_target);
}

template <bool EXACT>
hipError_t launch_view_gradient_samples(const ViewGradientArgs& a, hipStream_t stream)
{
    switch (a.samples) {
    case 1: return launch_view_gradient_flags<EXACT, 1>(a, stream);
    case 2: return launch_view_gradient_flags<EXACT, 2>(a, stream);
    case 4: return launch_view_gradient_flags<EXACT, 4>(a, stream);
    default: return hipErrorInvalidValue; // a missing kernel is an error
    }
}

} // namespace

hipError_t launch_view_gradient(const ViewGradientArgs& a, hipStream_t stream)
{
    if (a.walk.g.num_tiles <= 0) return hipErrorInvalidValue;
    const hipError_t e = a.walk.exact_exp ? launch_view_gradient_samples<true>(a, stream) : launch_view_gradient_samples<false>(a, stream);
    if (e != hipSuccess) return e;
    return launch_det_gather(a.walk, stream); // deterministic mode: the slots of the view's rectangles, summed in slot order into walk.grads
}

hipError_t launch_view_adjoint(const float* splats, const uint8_t* held, int n, ViewXform x, const float* view_grads, float* grads,
                               hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(view_adjoint_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, splats, held, n, x, view_grads, grads);
    return hipGetLastError();
}

} // namespace s2d
