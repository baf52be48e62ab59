// s2d_loss_weighted.hip -- the loss terms and dL/d(image0) under a per-pixel weight plane (s2d_loss_weighted.h,
// include/splat2d_weights.h): the entry points of the weighted pass, and the check of a candidate plane.
//
// The launches are those of s2d_loss.hip, kernel for kernel, and the bodies are the same ones (s2d_loss_kernels.h), here
// with the plane: omega on the stored maps and the pointwise terms, four sums.
//   wloss_moments_kernel, wloss_adjoint_kernel, wloss_pointwise_kernel   as their namesakes of s2d_loss.hip;
//   wloss_finalize_kernel   the four totals in the order of loss_finalize_kernel;
//   weight_check_kernel, weight_check_finish_kernel   is a candidate plane finite and >= 0, and what is its sum.
// The two units stay two: a unit's kernels have changed their register allocation before when instantiations were added
// beside them.
#include "s2d_loss_weighted.h"

#include "s2d_loss_kernels.h"

namespace s2d {

template <bool HALF>
__global__ __launch_bounds__(256) void wloss_moments_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                            const float* __restrict__ omega, int W, int H, int tiles_x, LossWindow win,
                                                            float* __restrict__ maps, double* __restrict__ partial, int slots, int want_l1,
                                                            const DeviceStatus* __restrict__ status, int iteration)
{
    loss_moments_body<HALF, true>(image0, image_ref, omega, W, H, tiles_x, win, maps, partial, slots, want_l1, status, iteration);
}

template <bool HALF>
__global__ __launch_bounds__(256) void wloss_adjoint_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                            const float* __restrict__ omega, int W, int H, int tiles_x, LossWindow win,
                                                            const float* __restrict__ maps, float w_mse, float w_l1, float w_dssim,
                                                            float4* __restrict__ dimage, const DeviceStatus* __restrict__ status,
                                                            int iteration)
{
    loss_adjoint_body<HALF, true>(image0, image_ref, omega, W, H, tiles_x, win, maps, w_mse, w_l1, w_dssim, dimage, status, iteration);
}

template <bool HALF>
__global__ __launch_bounds__(256) void wloss_pointwise_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                              const float* __restrict__ omega, size_t pixels, float w_mse, float w_l1,
                                                              float4* __restrict__ dimage, double* __restrict__ partial, int slots,
                                                              const DeviceStatus* __restrict__ status, int iteration)
{
    loss_pointwise_body<HALF, true>(image0, image_ref, omega, pixels, w_mse, w_l1, dimage, partial, slots, status, iteration);
}

// out4: all four totals; out3: the slot of the unweighted ring (terms 0, 2, 3).
__global__ __launch_bounds__(256) void wloss_finalize_kernel(const double* __restrict__ partial, int slots, int count, int mask,
                                                             double* __restrict__ out4, double* __restrict__ out3,
                                                             double* __restrict__ sqerr_out, const DeviceStatus* __restrict__ status,
                                                             int iteration)
{
    loss_finalize_body<kWeightedTerms>(partial, slots, count, mask, out4, out3, sqerr_out, status, iteration);
}

// 1024 consecutive values per workgroup: their sum and how many of them cannot be weights -> partial[2 * block], [2 * block + 1].
__global__ __launch_bounds__(256) void weight_check_kernel(const float* __restrict__ plane, size_t pixels, double* __restrict__ partial)
{
    __shared__ double red[4];
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    double a = 0.0, bad = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t i = base + (size_t)k * 256;
        if (i < pixels) {
            const float v = plane[i];
            if (v >= 0.0f && v <= 3.402823466e+38f) a += (double)v; // (NaN fails both comparisons)
            else bad += 1.0;
        }
    }
    const double t_a = block_sum_256(a, red), t_bad = block_sum_256(bad, red);
    if (threadIdx.x == 0) {
        partial[(size_t)2 * blockIdx.x] = t_a;
        partial[(size_t)2 * blockIdx.x + 1] = t_bad;
    }
}

__global__ __launch_bounds__(256) void weight_check_finish_kernel(const double* __restrict__ partial, size_t count, double* __restrict__ out2)
{
    __shared__ double s[4];
    double a = 0.0, bad = 0.0;
    for (size_t i = threadIdx.x; i < count; i += 256) {
        a += partial[2 * i];
        bad += partial[2 * i + 1];
    }
    const double t_a = block_sum_256(a, s), t_bad = block_sum_256(bad, s);
    if (threadIdx.x == 0) out2[0] = t_a, out2[1] = t_bad;
}

template <bool HALF>
static void launch_weighted_kernels(const WeightedLossArgs& wa, const LossWindow& win, int slots, int* count, hipStream_t stream)
{
    const LossArgs& a = wa.base;
    const int tiles_x = (a.W + kLossTile - 1) / kLossTile;
    if (a.w_dssim > 0.0f) {
        hipLaunchKernelGGL(wloss_moments_kernel<HALF>, dim3((unsigned)slots), dim3(256), 0, stream, a.image0, a.image_ref, wa.omega, a.W,
                           a.H, tiles_x, win, a.maps, wa.partial4, slots, a.w_l1 > 0.0f ? 1 : 0, a.status, a.iteration);
        hipLaunchKernelGGL(wloss_adjoint_kernel<HALF>, dim3((unsigned)slots), dim3(256), 0, stream, a.image0, a.image_ref, wa.omega, a.W,
                           a.H, tiles_x, win, (const float*)a.maps, a.w_mse, a.w_l1, a.w_dssim, a.dimage, a.status, a.iteration);
        *count = slots;
    } else {
        const size_t pixels = (size_t)a.W * (size_t)a.H;
        *count = (int)((pixels + 1023) / 1024); // <= slots
        hipLaunchKernelGGL(wloss_pointwise_kernel<HALF>, dim3((unsigned)*count), dim3(256), 0, stream, a.image0, a.image_ref, wa.omega,
                           pixels, a.w_mse, a.w_l1, a.dimage, wa.partial4, slots, a.status, a.iteration);
    }
}

hipError_t launch_loss_weighted(const WeightedLossArgs& wa, hipStream_t stream)
{
    const LossArgs& a = wa.base;
    const int slots = loss_slots(a.W, a.H);
    int count = 0;
    if (a.half_images) launch_weighted_kernels<true>(wa, loss_window(), slots, &count, stream);
    else launch_weighted_kernels<false>(wa, loss_window(), slots, &count, stream);
    const int mask = 3 | (a.w_l1 > 0.0f ? 4 : 0) | (a.w_dssim > 0.0f ? 8 : 0);
    hipLaunchKernelGGL(wloss_finalize_kernel, dim3(1), dim3(256), 0, stream, (const double*)wa.partial4, slots, count, mask, wa.out4,
                       a.out3, a.sqerr_out, a.status, a.iteration);
    return hipGetLastError();
}

hipError_t launch_weight_check(const float* plane, size_t pixels, double* partial, double* out2, hipStream_t stream)
{
    const size_t blocks = weight_check_slots(pixels);
    hipLaunchKernelGGL(weight_check_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, plane, pixels, partial);
    hipLaunchKernelGGL(weight_check_finish_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, blocks, out2);
    return hipGetLastError();
}

} // namespace s2d
