// s2d_loss.hip -- the loss terms and dL/d(image0) on the device (s2d_loss.h): the entry points of the
// plain pass.  The bodies are s2d_loss_kernels.h's, shared with the pass under a weight plane (s2d_loss_weighted.hip), here
// without the plane: nothing of it is read, nothing multiplied, three sums.
//
// With w_dssim > 0 a loss pass is three launches, one workgroup per 32 x 32 tile of the image in the first two:
//   loss_moments_kernel   the SSIM index and its three derivative maps, and the tile's double sums;
//   loss_adjoint_kernel   the window over the maps, plus the MSE and L1 terms -> the gradient image;
//   loss_finalize_kernel  the per-tile sums in a fixed order -> the loss ring (and the squared-error ring).
// With w_dssim == 0 no window kernel runs: loss_pointwise_kernel forms the gradient image and the sums, then the finalize.
#include "s2d_loss_kernels.h"

#include <cmath>

namespace s2d {

template <bool HALF>
__global__ __launch_bounds__(256) void loss_moments_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref, int W,
                                                           int H, int tiles_x, LossWindow win, float* __restrict__ maps,
                                                           double* __restrict__ partial, int slots, int want_l1,
                                                           const DeviceStatus* __restrict__ status, int iteration)
{
    loss_moments_body<HALF, false>(image0, image_ref, nullptr, W, H, tiles_x, win, maps, partial, slots, want_l1, status, iteration);
}

template <bool HALF>
__global__ __launch_bounds__(256) void loss_adjoint_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref, int W,
                                                           int H, int tiles_x, LossWindow win, const float* __restrict__ maps,
                                                           float w_mse, float w_l1, float w_dssim, float4* __restrict__ dimage,
                                                           const DeviceStatus* __restrict__ status, int iteration)
{
    loss_adjoint_body<HALF, false>(image0, image_ref, nullptr, W, H, tiles_x, win, maps, w_mse, w_l1, w_dssim, dimage, status, iteration);
}

template <bool HALF>
__global__ __launch_bounds__(256) void loss_pointwise_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                             size_t pixels, float w_mse, float w_l1, float4* __restrict__ dimage,
                                                             double* __restrict__ partial, int slots,
                                                             const DeviceStatus* __restrict__ status, int iteration)
{
    loss_pointwise_body<HALF, false>(image0, image_ref, nullptr, pixels, w_mse, w_l1, dimage, partial, slots, status, iteration);
}

__global__ __launch_bounds__(256) void loss_finalize_kernel(const double* __restrict__ partial, int slots, int count, int mask,
                                                            double* __restrict__ out3, double* __restrict__ sqerr_out,
                                                            const DeviceStatus* __restrict__ status, int iteration)
{
    loss_finalize_body<kLossTerms>(partial, slots, count, mask, out3, nullptr, sqerr_out, status, iteration);
}

const LossWindow& loss_window()
{
    static const LossWindow win = [] {
        double g[kLossTaps], sum = 0.0;
        for (int i = 0; i < kLossTaps; i++) sum += g[i] = std::exp(-(double)((i - kLossRadius) * (i - kLossRadius)) / (2.0 * 1.5 * 1.5));
        LossWindow w;
        for (int i = 0; i < kLossTaps; i++) w.g[i] = (float)(g[i] / sum);
        return w;
    }();
    return win;
}

template <bool HALF>
static void launch_loss_kernels(const LossArgs& a, const LossWindow& win, int slots, int* count, hipStream_t stream)
{
    const int tiles_x = (a.W + kLossTile - 1) / kLossTile;
    if (a.w_dssim > 0.0f) {
        hipLaunchKernelGGL(loss_moments_kernel<HALF>, dim3((unsigned)slots), dim3(256), 0, stream, a.image0, a.image_ref, a.W, a.H, tiles_x,
                           win, a.maps, a.partial, slots, a.w_l1 > 0.0f ? 1 : 0, a.status, a.iteration);
        hipLaunchKernelGGL(loss_adjoint_kernel<HALF>, dim3((unsigned)slots), dim3(256), 0, stream, a.image0, a.image_ref, a.W, a.H, tiles_x,
                           win, (const float*)a.maps, a.w_mse, a.w_l1, a.w_dssim, a.dimage, a.status, a.iteration);
        *count = slots;
    } else {
        const size_t pixels = (size_t)a.W * (size_t)a.H;
        *count = (int)((pixels + 1023) / 1024); // <= slots
        hipLaunchKernelGGL(loss_pointwise_kernel<HALF>, dim3((unsigned)*count), dim3(256), 0, stream, a.image0, a.image_ref, pixels, a.w_mse,
                           a.w_l1, a.dimage, a.partial, slots, a.status, a.iteration);
    }
}

hipError_t launch_loss(const LossArgs& a, hipStream_t stream)
{
    const int slots = loss_slots(a.W, a.H);
    int count = 0;
    if (a.half_images) launch_loss_kernels<true>(a, loss_window(), slots, &count, stream);
    else launch_loss_kernels<false>(a, loss_window(), slots, &count, stream);
    const int mask = 1 | (a.w_l1 > 0.0f ? 2 : 0) | (a.w_dssim > 0.0f ? 4 : 0);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, stream, (const double*)a.partial, slots, count, mask, a.out3,
                       a.sqerr_out, a.status, a.iteration);
    return hipGetLastError();
}

} // namespace s2d
