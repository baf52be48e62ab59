// s2d_loss.hip -- the loss terms and dL/d(image0) on the device (s2d_loss.h).
//
// With w_dssim > 0 a loss pass is three launches, one workgroup per 32 x 32 tile of the image in the first two:
//   loss_moments_kernel   x and y of one channel with a 5-pixel halo in LDS, a horizontal then a vertical 11-tap pass over
//                         x, y, x^2, y^2, xy -> the SSIM index and its three derivative maps (9 planes of scratch), and the
//                         tile's double sums of the squared error, |d| and 1 - s.
//   loss_adjoint_kernel   the same window over the three maps (it is symmetric: the adjoint of the correlation is the
//                         correlation), combined with x and y at the pixel, plus the MSE and L1 terms -> one RGBA32F store.
//   loss_finalize_kernel  the per-tile sums in a fixed order -> the loss ring (and the squared-error ring).
// With w_dssim == 0 no window kernel runs: loss_pointwise_kernel forms the gradient image and the sums, then the finalize.
// No atomics: every output word has one writer, every sum one order.
#include "s2d_loss.h"

#include <hip/hip_fp16.h>

#include <cmath>

namespace s2d {

constexpr int kHalo = kLossTile + 2 * kLossRadius; // 42: rows and columns of a tile with its halo
constexpr int kStride = kHalo + 1;                 // LDS row stride of the staged tile (odd: rows fall into different banks)
constexpr int kGroups = kLossTile / 4;             // a thread of a window pass forms 4 adjacent outputs from 14 inputs
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

template <bool HALF>
__device__ __forceinline__ float4 loss_load(const void* base, size_t i)
{
    if (HALF) {
        const uint2 v = reinterpret_cast<const uint2*>(base)[i];
        const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&v.x));
        const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&v.y));
        return make_float4(a.x, a.y, b.x, b.y);
    }
    return reinterpret_cast<const float4*>(base)[i];
}

__device__ __forceinline__ float chan(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : v.z; }

__device__ __forceinline__ float sign0(float d) { return d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : 0.0f; } // sign(0) = 0; NaN -> 0

// 4 adjacent outputs of the 11-tap window from 14 inputs, taps added in ascending order.
__device__ __forceinline__ void window4(const float (&v)[14], const LossWindow& win, float (&out)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float acc = win.g[0] * v[k];
#pragma unroll
        for (int j = 1; j < kLossTaps; j++) acc += win.g[j] * v[k + j];
        out[k] = acc;
    }
}

// The squared error of a pixel as main.cpp:801-802 forms it (float per pixel), and |d| of its three channels (exact in double).
__device__ __forceinline__ void pixel_terms(const float4& x, const float4& y, bool want_l1, double& a_sq, double& a_l1)
{
    const float ex = (x.x - y.x) * 255.0f, ey = (x.y - y.y) * 255.0f, ez = (x.z - y.z) * 255.0f;
    a_sq += (double)(ex * ex + ey * ey + ez * ez);
    if (want_l1) a_l1 += (fabs((double)x.x - (double)y.x) + fabs((double)x.y - (double)y.y)) + fabs((double)x.z - (double)y.z);
}

// partial[t * slots + slot], t = 0 squared error, 1 sum |d|, 2 sum (1 - s): one fixed order within the workgroup
__device__ __forceinline__ void store_partials(double a_sq, double a_l1, double a_ds, double* __restrict__ partial, int slots, int slot,
                                               double* s4)
{
    const double t_sq = block_sum_256(a_sq, s4), t_l1 = block_sum_256(a_l1, s4), t_ds = block_sum_256(a_ds, s4);
    if (threadIdx.x == 0) {
        partial[slot] = t_sq;
        partial[(size_t)slots + slot] = t_l1;
        partial[(size_t)2 * slots + slot] = t_ds;
    }
}

template <bool HALF>
__global__ __launch_bounds__(256) void loss_moments_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref, int W,
                                                           int H, int tiles_x, LossWindow win, float* __restrict__ maps,
                                                           double* __restrict__ partial, int slots, int want_l1,
                                                           const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ float sx[kHalo * kStride], sy[kHalo * kStride]; // one channel of x and y, zero outside the image
    __shared__ float hb[5][kHalo * kLossTile];                 // after the horizontal pass: x, y, x^2, y^2, xy
    __shared__ double red[4];
    if (status->first_nonfinite_iter < iteration) return; // the reference abort()ed in an earlier iteration
    const int tid = (int)threadIdx.x, tile = (int)blockIdx.x;
    const int tx0 = (tile % tiles_x) * kLossTile, ty0 = (tile / tiles_x) * kLossTile;
    const size_t plane = (size_t)W * (size_t)H;
    // the thread's own pixels: column tid & 31, rows (tid >> 5) * 4 + k
    const int col = tid & 31, r4 = (tid >> 5) * 4;
    const int px = tx0 + col, py0 = ty0 + r4;

    double a_sq = 0.0, a_l1 = 0.0, a_ds = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (px < W && py0 + k < H) {
            const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
            pixel_terms(loss_load<HALF>(image0, i), loss_load<HALF>(image_ref, i), want_l1 != 0, a_sq, a_l1);
        }
    }

#pragma unroll
    for (int c = 0; c < 3; c++) {
        // (sx / sy were last read before the barrier that closed the previous channel's horizontal pass)
        for (int i = tid; i < kHalo * kHalo; i += 256) {
            const int r = i / kHalo, q = i - r * kHalo;
            const int gx = tx0 - kLossRadius + q, gy = ty0 - kLossRadius + r;
            float vx = 0.0f, vy = 0.0f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t idx = (size_t)gy * (size_t)W + (size_t)gx;
                vx = chan(loss_load<HALF>(image0, idx), c);
                vy = chan(loss_load<HALF>(image_ref, idx), c);
            }
            sx[r * kStride + q] = vx;
            sy[r * kStride + q] = vy;
        }
        __syncthreads(); // (every thread is also through the previous channel's vertical pass: hb is free)
        for (int item = tid; item < kHalo * kGroups; item += 256) {
            const int r = item / kGroups, c0 = (item - r * kGroups) * 4;
            float vx[14], vy[14], t[14], o[4];
#pragma unroll
            for (int j = 0; j < 14; j++) {
                vx[j] = sx[r * kStride + c0 + j];
                vy[j] = sy[r * kStride + c0 + j];
            }
            const int dst = r * kLossTile + c0;
            window4(vx, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[0][dst + k] = o[k];
            window4(vy, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[1][dst + k] = o[k];
#pragma unroll
            for (int j = 0; j < 14; j++) t[j] = vx[j] * vx[j];
            window4(t, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[2][dst + k] = o[k];
#pragma unroll
            for (int j = 0; j < 14; j++) t[j] = vy[j] * vy[j];
            window4(t, win, o);
#pragma unroll
            for (int k = 0; k < 4; k++) hb[3][dst + k] = o[k];
#pragma unroll
            for (int j = 0; j < 14; j++) t[j] = vx[j] * vy[j];
            window4(t, win, o);
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
            window4(v, win, mom[m]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (px < W && py0 + k < H) {
                const float mux = mom[0][k], muy = mom[1][k];
                const float mx2 = mux * mux, my2 = muy * muy, mxy = mux * muy;
                const float sxx = mom[2][k] - mx2, syy = mom[3][k] - my2, sxy = mom[4][k] - mxy;
                const float A1 = 2.0f * mxy + kC1, A2 = 2.0f * sxy + kC2;
                const float B1 = (mx2 + my2) + kC1, B2 = (sxx + syy) + kC2; // >= C1, ~>= C2: never 0
                const float D = B1 * B2, invD = 1.0f / D;
                const float s = (A1 * A2) / D;
                a_ds += (double)(1.0f - s);
                // derivatives of 1 - s with respect to mu_x (through the variances too), w*x^2 and w*xy; y is fixed
                const float mA = (2.0f * muy * (A1 - A2) + 2.0f * mux * s * (B2 - B1)) * invD;
                const float mB = s / B2;
                const float mC = -2.0f * A1 * invD;
                const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
                maps[(size_t)(c * 3 + 0) * plane + i] = mA;
                maps[(size_t)(c * 3 + 1) * plane + i] = mB;
                maps[(size_t)(c * 3 + 2) * plane + i] = mC;
            }
        }
    }
    store_partials(a_sq, a_l1, a_ds, partial, slots, tile, red);
}

template <bool HALF>
__global__ __launch_bounds__(256) void loss_adjoint_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref, int W,
                                                           int H, int tiles_x, LossWindow win, const float* __restrict__ maps,
                                                           float w_mse, float w_l1, float w_dssim, float4* __restrict__ dimage,
                                                           const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ float sm[3][kHalo * kStride];   // the three maps of one channel, zero outside the image
    __shared__ float hb[3][kHalo * kLossTile]; // after the horizontal pass
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
            x[k] = loss_load<HALF>(image0, i);
            y[k] = loss_load<HALF>(image_ref, i);
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
            window4(v, win, o);
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
            window4(v, win, t[m]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) g[k][c] = (t[0][k] + (2.0f * chan(x[k], c)) * t[1][k]) + chan(y[k], c) * t[2][k];
    }

#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (px < W && py0 + k < H) {
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = chan(x[k], c) - chan(y[k], c);
                float v = w_dssim * g[k][c];
                if (w_mse > 0.0f) v += w_mse * d;
                if (w_l1 > 0.0f) v += w_l1 * sign0(d);
                o[c] = v;
            }
            dimage[(size_t)(py0 + k) * (size_t)W + (size_t)px] = make_float4(o[0], o[1], o[2], 0.0f);
        }
    }
}

// w_dssim == 0: the gradient image and the sums of 1024 consecutive pixels per workgroup.  With weights (1, 0, 0) a channel
// is 1.0f * (x - y): the subtraction of main.cpp:616 and nothing else.
template <bool HALF>
__global__ __launch_bounds__(256) void loss_pointwise_kernel(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                             size_t pixels, float w_mse, float w_l1, float4* __restrict__ dimage,
                                                             double* __restrict__ partial, int slots,
                                                             const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ double red[4];
    if (status->first_nonfinite_iter < iteration) return;
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    double a_sq = 0.0, a_l1 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t i = base + (size_t)k * 256;
        if (i < pixels) {
            const float4 x = loss_load<HALF>(image0, i), y = loss_load<HALF>(image_ref, i);
            pixel_terms(x, y, w_l1 > 0.0f, a_sq, a_l1);
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = chan(x, c) - chan(y, c);
                float v = 0.0f;
                if (w_mse > 0.0f) v = w_mse * d;
                if (w_l1 > 0.0f) v = w_mse > 0.0f ? v + w_l1 * sign0(d) : w_l1 * sign0(d);
                o[c] = v;
            }
            dimage[i] = make_float4(o[0], o[1], o[2], 0.0f);
        }
    }
    store_partials(a_sq, a_l1, 0.0, partial, slots, (int)blockIdx.x, red);
}

// The totals of the terms in `mask` (bit t = term t), one workgroup, one fixed order: thread t adds slots t, t + 256, ...,
// then the block sum -- the pattern of sqerr_sum_small without its limit on the number of slots.
__global__ __launch_bounds__(256) void loss_finalize_kernel(const double* __restrict__ partial, int slots, int count, int mask,
                                                            double* __restrict__ out3, double* __restrict__ sqerr_out,
                                                            const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ double s[4];
    if (status->first_nonfinite_iter < iteration) return;
    for (int t = 0; t < 3; t++) {
        if (!((mask >> t) & 1)) continue; // block-uniform
        double a = 0.0;
        for (int i = (int)threadIdx.x; i < count; i += 256) a += partial[(size_t)t * slots + i];
        const double total = block_sum_256(a, s);
        if (threadIdx.x == 0) {
            out3[t] = total;
            if (t == 0 && sqerr_out) *sqerr_out = total;
        }
    }
}

static LossWindow make_window()
{
    double g[kLossTaps], sum = 0.0;
    for (int i = 0; i < kLossTaps; i++) sum += g[i] = std::exp(-(double)((i - kLossRadius) * (i - kLossRadius)) / (2.0 * 1.5 * 1.5));
    LossWindow w;
    for (int i = 0; i < kLossTaps; i++) w.g[i] = (float)(g[i] / sum);
    return w;
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
    static const LossWindow win = make_window();
    const int slots = loss_slots(a.W, a.H);
    int count = 0;
    if (a.half_images) launch_loss_kernels<true>(a, win, slots, &count, stream);
    else launch_loss_kernels<false>(a, win, slots, &count, stream);
    const int mask = 1 | (a.w_l1 > 0.0f ? 2 : 0) | (a.w_dssim > 0.0f ? 4 : 0);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, stream, (const double*)a.partial, slots, count, mask, a.out3,
                       a.sqerr_out, a.status, a.iteration);
    return hipGetLastError();
}

} // namespace s2d
