// s2d_view_fit.hip -- the kernels of coarse-to-fine fitting (include/splat2d_coarse.h): view_fit_kernel, one
// iteration's pass through a view against a target of the view's size -- view_gradient_kernel<..., FROM_TARGET = true>
// (s2d_view_gradient.hip) with the squared error of the view riding along -- and view_target_kernel, which resamples the context's
// target to a view's window (s2d_view_target_math.h).
//
// view_fit_kernel is composed exactly as its sibling is, of the same pieces (s2d_view_walk.h): forward_tile, view_top_lane,
// view_minus_target (the resolve in lanes, then resolved - target in the top-left lane of an output pixel), view_broadcast (times
// 0.25 per level), view_zero_outside, backward_tile (UPSTREAM).  One step of its own stands between view_minus_target and the
// broadcast: the top-left lane's term (dx * 255)^2 + (dy * 255)^2 +
// (dz * 255)^2, a float, as pixel_terms (s2d_loss.hip) and main.cpp:801-802 form it -- every other lane contributes 0 -- is summed
// over the workgroup in double (block_sum_256) and stored, one plain store, to tile_sqerr[tile].  A tile whose list is empty, or
// none of whose entries executes, stores the energy of its piece of the target like any other.  The four doubles of the sum lie
// in the LDS the two walks share: the forward walk is done with it behind the barrier that used to stand before the backward
// walk, and block_sum_256 ends with the barrier the backward walk needs.  The per-tile values are added up in a fixed order by
// sqerr_reduce (launch_sqerr_finalize), as the training image's are.
// The gradients are the bytes view_gradient_kernel gives: nothing that reaches backward_tile differs.
#include "s2d_view_walk.h"
#include "s2d_view_target_math.h"
#include "s2d_walk_backward.h"

namespace s2d {

template <bool EXACT, int S, bool NEED_OP, bool DET>
__global__ __launch_bounds__(256, (EXACT && DET) ? 4 : 8) void view_fit_kernel(const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ list,
                                                          const ProjRec* __restrict__ proj, const float4* __restrict__ target,
                                                          unsigned long long* __restrict__ wave_masks,
                                                          uint32_t* __restrict__ exec_list, uint32_t* __restrict__ tile_exec,
                                                          uint32_t* __restrict__ retire_hint, float* __restrict__ grads,
                                                          double* __restrict__ tile_sqerr, Geometry g, int out_width, DetSlots det)
{
    static_assert(S == 1 || S == 2 || S == 4, "samples per axis");
    constexpr size_t kBytes = sizeof(BwdShared<DET>) > sizeof(FwdShared) ? sizeof(BwdShared<DET>) : sizeof(FwdShared);
    static_assert(kBytes >= 4 * sizeof(double), "the block sum's four doubles");
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes]; // the two walks and the block sum between them use the same LDS
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
    float4 u = view_minus_target<S>(fin, top, target, o);
    double e2 = 0.0;
    if (top) {
        const float ex = u.x * 255.0f, ey = u.y * 255.0f, ez = u.z * 255.0f; // main.cpp:801-802: float per pixel, double across pixels
        e2 = (double)(ex * ex + ey * ey + ez * ez);
    }
    // the sum, and behind it the backward walk, re-use the LDS the forward walk's hand-over may still be reading; the backward
    // walk reads what other threads of the workgroup handed over through global memory
    __syncthreads();
    const double tile_e2 = block_sum_256(e2, reinterpret_cast<double*>(smem));
    if (c.tid == 0) tile_sqerr[tile] = tile_e2;
    view_broadcast<S>(u, c.lane);
    view_zero_outside(c, fin, u);
    backward_tile<false, NEED_OP, DET, EXACT, false, true>(*reinterpret_cast<BwdShared<DET>*>(smem), c, fin, u, tile_off, list, proj,
                                                           wave_masks, exec_list, n_exec, grads, nullptr, g, det, nullptr,
                                                           SqerrJob{nullptr, 0, nullptr, nullptr});
}

// One thread per output pixel: view_target_pixel of the context's target (fp16 targets converted to fp32 as they are loaded).
struct TargetLoad {
    const void* ref;
    int W;
    int half;
    __device__ __forceinline__ void operator()(int x, int y, float* t) const
    {
        const size_t i = (size_t)y * (size_t)W + (size_t)x;
        const float4 v = half ? load_pixel<true>(ref, i) : load_pixel<false>(ref, i);
        t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
    }
};

__global__ __launch_bounds__(256) void view_target_kernel(const void* __restrict__ ref, int half, int W, int H, float origin_x, float origin_y,
                                                          float zoom, int out_width, int out_height, float4* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (size_t)out_width * (size_t)out_height) return;
    const int j = (int)(p / (size_t)out_width), i = (int)(p % (size_t)out_width);
    float v[4];
    view_target_pixel(TargetLoad{ref, W, half}, W, H, origin_x, origin_y, zoom, i, j, v);
    out[p] = make_float4(v[0], v[1], v[2], v[3]);
}

hipError_t launch_view_fit(const ViewGradientArgs& a, hipStream_t stream)
{
    const RasterArgs& w = a.walk;
    if (w.g.num_tiles <= 0 || w.tile_sqerr == nullptr || a.src == nullptr || !a.from_target) return hipErrorInvalidValue;
    const dim3 grid((unsigned)w.g.num_tiles), block(256);
    const std::false_type no; // flags the view has no variants of: pair counting, fp16 images
    const hipError_t e = with_samples(a.samples, [&](auto samples) {
        constexpr int S = decltype(samples)::value;
        return with_variant([&](auto exact, auto, auto, auto op, auto d) {
            hipLaunchKernelGGL((view_fit_kernel<exact, S, op, d>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.src, w.wave_masks,
                               w.exec_list, w.tile_exec, w.retire_hint, w.grads, w.tile_sqerr, w.g, a.out_width, det_slots(w.det));
        }, w.exact_exp, no, no, w.need_opacity_grad, w.det.now != 0u);
    });
    if (e != hipSuccess) return e;
    return launch_det_gather(w, stream); // deterministic mode: the slots of the view's rectangles, summed in slot order into walk.grads
}

hipError_t launch_view_target(const void* ref, bool half_images, int W, int H, float origin_x, float origin_y, float zoom, int out_width,
                              int out_height, float4* out, hipStream_t stream)
{
    const size_t pixels = (size_t)out_width * (size_t)out_height;
    if (pixels == 0 || ref == nullptr || out == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(view_target_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, ref, half_images ? 1 : 0, W, H,
                       origin_x, origin_y, zoom, out_width, out_height, out);
    return hipGetLastError();
}

} // namespace s2d
