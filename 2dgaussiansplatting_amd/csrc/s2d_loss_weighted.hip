// s2d_loss_weighted.hip -- the loss terms and dL/d(image0) under a per-pixel weight plane (s2d_loss_weighted.h,
// include/splat2d_weights.h).
//
// The launches are those of s2d_loss.hip, kernel for kernel, and so is the arithmetic up to the one place omega enters:
//   wloss_moments_kernel    stores omega * mA, omega * mB, omega * mC (the weight of the D-SSIM term sits at the window's
//                           CENTRE, so it multiplies the maps before the adjoint correlation), and the tile's four double sums;
//   wloss_adjoint_kernel    v = w_dssim * g as ever, then v += omega * (w_mse * d), then v += omega * (w_l1 * sign0(d));
//   wloss_pointwise_kernel  the same without the first term (w_dssim == 0);
//   wloss_finalize_kernel   the four totals in the order of loss_finalize_kernel;
//   weight_check_kernel, weight_check_finish_kernel   is a candidate plane finite and >= 0, and what is its sum.
// A sum's addend is (double)omega * (double)term, term being what the unweighted kernel adds: a plane of ones adds the same
// doubles in the same order.  The window code is restated here rather than shared through a header, so that s2d_loss.hip's
// kernels stay instruction for instruction what they are.  omega is read where it is used, behind the window passes: the
// registers of the passes are those of the unweighted kernels.  No atomics: every output word has one writer.
#include "s2d_loss_weighted.h"

#include <hip/hip_fp16.h>

#include <cmath>

namespace s2d {

constexpr int kHalo = kLossTile + 2 * kLossRadius; // 42
constexpr int kStride = kHalo + 1;
constexpr int kGroups = kLossTile / 4;
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

template <bool HALF>
__device__ __forceinline__ float4 wl_load(const void* base, size_t i)
{
    if (HALF) {
        const uint2 v = reinterpret_cast<const uint2*>(base)[i];
        const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&v.x));
        const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&v.y));
        return make_float4(a.x, a.y, b.x, b.y);
    }
    return reinterpret_cast<const float4*>(base)[i];
}

__device__ __forceinline__ float wl_chan(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : v.z; }

__device__ __forceinline__ float wl_sign0(float d) { return d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : 0.0f; }

// 4 adjacent outputs of the 11-tap window from 14 inputs, taps added in ascending order (window4 of s2d_loss.hip).
__device__ __forceinline__ void wl_window4(const float (&v)[14], const LossWindow& win, float (&out)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float acc = win.g[0] * v[k];
#pragma unroll
        for (int j = 1; j < kLossTaps; j++) acc += win.g[j] * v[k + j];
        out[k] = acc;
    }
}

// The terms of one pixel as pixel_terms of s2d_loss.hip forms them, then once more under the pixel's weight.
__device__ __forceinline__ void wl_pixel_terms(const float4& x, const float4& y, float om, bool want_l1, double& a_sq, double& a_wsq,
                                               double& a_wl1)
{
    const float ex = (x.x - y.x) * 255.0f, ey = (x.y - y.y) * 255.0f, ez = (x.z - y.z) * 255.0f;
    const double sq = (double)(ex * ex + ey * ey + ez * ez);
    a_sq += sq;
    a_wsq += (double)om * sq;
    if (want_l1) a_wl1 += (double)om * ((fabs((double)x.x - (double)y.x) + fabs((double)x.y - (double)y.y)) + fabs((double)x.z - (double)y.z));
}

// partial[t * slots + slot], t = 0 squared error, 1 omega * squared error, 2 omega * |d|, 3 omega * (1 - s)
__device__ __forceinline__ void wl_store_partials(double a_sq, double a_wsq, double a_wl1, double a_wds, double* __restrict__ partial,
                                                  int slots, int slot, double* s4)
{
    const double t_sq = block_sum_256(a_sq, s4), t_wsq = block_sum_256(a_wsq, s4);
    const double t_wl1 = block_sum_256(a_wl1, s4), t_wds = block_sum_256(a_wds, s4);
    if (threadIdx.x == 0) {
        partial[slot] = t_sq;
        partial[(size_t)slots + slot] = t_wsq;
        partial[(size_t)2 * slots + slot] = t_wl1;
        partial[(size_t)3 * slots + slot] = t_wds;
    }
}

template <bool HALF>
__global__ __launch_bounds__(256) void wloss_moments_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                            const float* __restrict__ omega, int W, int H, int tiles_x, LossWindow win,
                                                            float* __restrict__ maps, double* __restrict__ partial, int slots, int want_l1,
                                                            const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ float sx[kHalo * kStride], sy[kHalo * kStride];
    __shared__ float hb[5][kHalo * kLossTile];
    __shared__ double red[4];
    if (status->first_nonfinite_iter < iteration) return;
    const int tid = (int)threadIdx.x, tile = (int)blockIdx.x;
    const int tx0 = (tile % tiles_x) * kLossTile, ty0 = (tile / tiles_x) * kLossTile;
    const size_t plane = (size_t)W * (size_t)H;
    const int col = tid & 31, r4 = (tid >> 5) * 4;
    const int px = tx0 + col, py0 = ty0 + r4;

    double a_sq = 0.0, a_wsq = 0.0, a_wl1 = 0.0, a_wds = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (px < W && py0 + k < H) {
            const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
            wl_pixel_terms(wl_load<HALF>(image0, i), wl_load<HALF>(image_ref, i), omega[i], want_l1 != 0, a_sq, a_wsq, a_wl1);
        }
    }

#pragma unroll
    for (int c = 0; c < 3; c++) {
        for (int i = tid; i < kHalo * kHalo; i += 256) {
            const int r = i / kHalo, q = i - r * kHalo;
            const int gx = tx0 - kLossRadius + q, gy = ty0 - kLossRadius + r;
            float vx = 0.0f, vy = 0.0f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t idx = (size_t)gy * (size_t)W + (size_t)gx;
                vx = wl_chan(wl_load<HALF>(image0, idx), c);
                vy = wl_chan(wl_load<HALF>(image_ref, idx), c);
            }
            sx[r * kStride + q] = vx;
            sy[r * kStride + q] = vy;
        }
        __syncthreads();
        for (int item = tid; item < kHalo * kGroups; item += 256) {
            const int r = item / kGroups, c0 = (item - r * kGroups) * 4;
            float vx[14], vy[14], t[14], o[4];
#pragma unroll
            for (int j = 0; j < 14; j++) {
                vx[j] = sx[r * kStride + c0 + j];
                vy[j] = sy[r * kStride + c0 + j];
            }
            const int dst = r * kLossTile + c0;
            wl_window4(vx, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[0][dst + k] = o[k];
            wl_window4(vy, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[1][dst + k] = o[k];
#pragma unroll
            for (int j = 0; j < 14; j++) t[j] = vx[j] * vx[j];
            wl_window4(t, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[2][dst + k] = o[k];
#pragma unroll
            for (int j = 0; j < 14; j++) t[j] = vy[j] * vy[j];
            wl_window4(t, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[3][dst + k] = o[k];
#pragma unroll
            for (int j = 0; j < 14; j++) t[j] = vx[j] * vy[j];
            wl_window4(t, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[4][dst + k] = o[k];
        }
        __syncthreads();
        float mom[5][4];
#pragma unroll
        for (int m = 0; m < 5; m++) {
            float v[14];
#pragma unroll
            for (int j = 0; j < 14; j++) v[j] = hb[m][(r4 + j) * kLossTile + col];
            wl_window4(v, win, mom[m]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (px < W && py0 + k < H) {
                const float mux = mom[0][k], muy = mom[1][k];
                const float mx2 = mux * mux, my2 = muy * muy, mxy = mux * muy;
                const float sxx = mom[2][k] - mx2, syy = mom[3][k] - my2, sxy = mom[4][k] - mxy;
                const float A1 = 2.0f * mxy + kC1, A2 = 2.0f * sxy + kC2;
                const float B1 = (mx2 + my2) + kC1, B2 = (sxx + syy) + kC2;
                const float D = B1 * B2, invD = 1.0f / D;
                const float s = (A1 * A2) / D;
                const float mA = (2.0f * muy * (A1 - A2) + 2.0f * mux * s * (B2 - B1)) * invD;
                const float mB = s / B2;
                const float mC = -2.0f * A1 * invD;
                const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
                const float om = omega[i]; // (read here, behind the window passes; the line is in the cache since the pixel terms)
                a_wds += (double)om * (double)(1.0f - s);
                maps[(size_t)(c * 3 + 0) * plane + i] = om * mA;
                maps[(size_t)(c * 3 + 1) * plane + i] = om * mB;
                maps[(size_t)(c * 3 + 2) * plane + i] = om * mC;
            }
        }
    }
    wl_store_partials(a_sq, a_wsq, a_wl1, a_wds, partial, slots, tile, red);
}

template <bool HALF>
__global__ __launch_bounds__(256) void wloss_adjoint_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                            const float* __restrict__ omega, int W, int H, int tiles_x, LossWindow win,
                                                            const float* __restrict__ maps, float w_mse, float w_l1, float w_dssim,
                                                            float4* __restrict__ dimage, const DeviceStatus* __restrict__ status,
                                                            int iteration)
{
    __shared__ float sm[3][kHalo * kStride];
    __shared__ float hb[3][kHalo * kLossTile];
    if (status->first_nonfinite_iter < iteration) return;
    const int tid = (int)threadIdx.x, tile = (int)blockIdx.x;
    const int tx0 = (tile % tiles_x) * kLossTile, ty0 = (tile / tiles_x) * kLossTile;
    const size_t plane = (size_t)W * (size_t)H;
    const int col = tid & 31, r4 = (tid >> 5) * 4;
    const int px = tx0 + col, py0 = ty0 + r4;

    float4 x[4], y[4];
    float g[4][3];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        x[k] = y[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (px < W && py0 + k < H) {
            const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
            x[k] = wl_load<HALF>(image0, i);
            y[k] = wl_load<HALF>(image_ref, i);
        }
    }

#pragma unroll
    for (int c = 0; c < 3; c++) {
        for (int i = tid; i < kHalo * kHalo; i += 256) {
            const int r = i / kHalo, q = i - r * kHalo;
            const int gx = tx0 - kLossRadius + q, gy = ty0 - kLossRadius + r;
            float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t idx = (size_t)gy * (size_t)W + (size_t)gx;
                v0 = maps[(size_t)(c * 3 + 0) * plane + idx];
                v1 = maps[(size_t)(c * 3 + 1) * plane + idx];
                v2 = maps[(size_t)(c * 3 + 2) * plane + idx];
            }
            sm[0][r * kStride + q] = v0;
            sm[1][r * kStride + q] = v1;
            sm[2][r * kStride + q] = v2;
        }
        __syncthreads();
        for (int item = tid; item < 3 * kHalo * kGroups; item += 256) {
            const int m = item / (kHalo * kGroups), rem = item - m * (kHalo * kGroups);
            const int r = rem / kGroups, c0 = (rem - r * kGroups) * 4;
            float v[14], o[4];
#pragma unroll
            for (int j = 0; j < 14; j++) v[j] = sm[m][r * kStride + c0 + j];
            wl_window4(v, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[m][r * kLossTile + c0 + k] = o[k];
        }
        __syncthreads();
        float t[3][4];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            float v[14];
#pragma unroll
            for (int j = 0; j < 14; j++) v[j] = hb[m][(r4 + j) * kLossTile + col];
            wl_window4(v, win, t[m]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) g[k][c] = (t[0][k] + (2.0f * wl_chan(x[k], c)) * t[1][k]) + wl_chan(y[k], c) * t[2][k];
    }

#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (px < W && py0 + k < H) {
            const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
            const float om = omega[i]; // the one read of the plane, behind everything else
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = wl_chan(x[k], c) - wl_chan(y[k], c);
                float v = w_dssim * g[k][c];
                if (w_mse > 0.0f) v += om * (w_mse * d);
                if (w_l1 > 0.0f) v += om * (w_l1 * wl_sign0(d));
                o[c] = v;
            }
            dimage[i] = make_float4(o[0], o[1], o[2], 0.0f);
        }
    }
}

template <bool HALF>
__global__ __launch_bounds__(256) void wloss_pointwise_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                              const float* __restrict__ omega, size_t pixels, float w_mse, float w_l1,
                                                              float4* __restrict__ dimage, double* __restrict__ partial, int slots,
                                                              const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ double red[4];
    if (status->first_nonfinite_iter < iteration) return;
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    double a_sq = 0.0, a_wsq = 0.0, a_wl1 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t i = base + (size_t)k * 256;
        if (i < pixels) {
            const float4 x = wl_load<HALF>(image0, i), y = wl_load<HALF>(image_ref, i);
            const float om = omega[i];
            wl_pixel_terms(x, y, om, w_l1 > 0.0f, a_sq, a_wsq, a_wl1);
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = wl_chan(x, c) - wl_chan(y, c);
                float v = 0.0f;
                if (w_mse > 0.0f) v = om * (w_mse * d);
                if (w_l1 > 0.0f) v = w_mse > 0.0f ? v + om * (w_l1 * wl_sign0(d)) : om * (w_l1 * wl_sign0(d));
                o[c] = v;
            }
            dimage[i] = make_float4(o[0], o[1], o[2], 0.0f);
        }
    }
    wl_store_partials(a_sq, a_wsq, a_wl1, 0.0, partial, slots, (int)blockIdx.x, red);
}

// The totals of the terms in `mask` (bit t = term t of the four), one workgroup, the order of loss_finalize_kernel: thread t
// adds slots t, t + 256, ..., then the block sum.  out4: all four; out3: the slot of the unweighted ring (terms 0, 2, 3).
__global__ __launch_bounds__(256) void wloss_finalize_kernel(const double* __restrict__ partial, int slots, int count, int mask,
                                                             double* __restrict__ out4, double* __restrict__ out3,
                                                             double* __restrict__ sqerr_out, const DeviceStatus* __restrict__ status,
                                                             int iteration)
{
    __shared__ double s[4];
    if (status->first_nonfinite_iter < iteration) return;
    for (int t = 0; t < kWeightedTerms; t++) {
        if (!((mask >> t) & 1)) continue; // block-uniform
        double a = 0.0;
        for (int i = (int)threadIdx.x; i < count; i += 256) a += partial[(size_t)t * slots + i];
        const double total = block_sum_256(a, s);
        if (threadIdx.x == 0) {
            out4[t] = total;
            if (t != 1) out3[t == 0 ? 0 : t - 1] = total;
            if (t == 0 && sqerr_out) *sqerr_out = total;
        }
    }
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

static LossWindow make_weighted_window()
{
    double g[kLossTaps], sum = 0.0;
    for (int i = 0; i < kLossTaps; i++) sum += g[i] = std::exp(-(double)((i - kLossRadius) * (i - kLossRadius)) / (2.0 * 1.5 * 1.5));
    LossWindow w;
    for (int i = 0; i < kLossTaps; i++) w.g[i] = (float)(g[i] / sum);
    return w;
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
    static const LossWindow win = make_weighted_window();
    const LossArgs& a = wa.base;
    const int slots = loss_slots(a.W, a.H);
    int count = 0;
    if (a.half_images) launch_weighted_kernels<true>(wa, win, slots, &count, stream);
    else launch_weighted_kernels<false>(wa, win, slots, &count, stream);
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
