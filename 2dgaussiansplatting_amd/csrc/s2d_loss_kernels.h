// s2d_loss_kernels.h -- the bodies of the loss kernels, once, for the plain pass (s2d_loss.hip) and the pass under a
// per-pixel weight plane (s2d_loss_weighted.hip); DESIGN.md sections 13 and 26.  The two units hold the __global__ entry
// points and nothing of the arithmetic.
//
//   loss_moments_body    x and y of one channel with a 5-pixel halo in LDS, a horizontal then a vertical 11-tap pass over
//                        x, y, x^2, y^2, xy -> the SSIM index and its three derivative maps (9 planes of scratch), and the
//                        tile's double sums.
//   loss_adjoint_body    the same window over the three maps (it is symmetric: the adjoint of the correlation is the
//                        correlation), combined with x and y at the pixel, plus the MSE and L1 terms -> one RGBA32F store.
//   loss_pointwise_body  w_dssim == 0: no window, the gradient image and the sums of 1024 consecutive pixels per workgroup.
//   loss_finalize_body   the per-tile sums in a fixed order -> the totals.
// WEIGHTED: omega multiplies the three stored map values (the weight of the D-SSIM term sits at the window's CENTRE, so it
// stands before the adjoint correlation) and each pointwise term of the gradient, v += omega * (w_mse * d); a sum's addend is
// (double)omega * (double)term, and the unweighted squared error is kept beside the weighted one: kWeightedTerms sums instead
// of kLossTerms.  omega is read where it is used, behind the window passes.  Without WEIGHTED no plane is read and nothing
// is multiplied.  The build contracts nothing (-ffp-contract=off), so a written word follows from the order of the
// operations below alone: a plane of ones adds the same doubles in the same order and stores the same floats.
// No atomics: every output word has one writer, every sum one order.
#pragma once

#include "s2d_loss.h"

#include <hip/hip_fp16.h>

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

// A term of the gradient or a stored map value under the pixel's weight: om * term, or without a plane the term as it is.
template <bool WEIGHTED>
__device__ __forceinline__ float under(float om, float term) { return WEIGHTED ? om * term : term; }

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

// The sums a thread carries through a pass.  Without a plane wsq stays untouched and l1, ds are the plain sums.
struct LossSums {
    double sq = 0.0;  // the squared error of main.cpp:801-802 (255 scale), never weighted
    double wsq = 0.0; // omega * that
    double l1 = 0.0;  // (omega *) |d| of the three channels
    double ds = 0.0;  // (omega *) (1 - s)
};

// The squared error of a pixel as main.cpp:801-802 forms it (float per pixel), and |d| of its three channels (exact in double).
template <bool WEIGHTED>
__device__ __forceinline__ void pixel_terms(const float4& x, const float4& y, float om, bool want_l1, LossSums& a)
{
    const float ex = (x.x - y.x) * 255.0f, ey = (x.y - y.y) * 255.0f, ez = (x.z - y.z) * 255.0f;
    const double sq = (double)(ex * ex + ey * ey + ez * ez);
    a.sq += sq;
    if (WEIGHTED) a.wsq += (double)om * sq;
    if (want_l1) {
        const double l1 = (fabs((double)x.x - (double)y.x) + fabs((double)x.y - (double)y.y)) + fabs((double)x.z - (double)y.z);
        a.l1 += WEIGHTED ? (double)om * l1 : l1;
    }
}

// partial[t * slots + slot]: t = 0 squared error, 1 sum |d|, 2 sum (1 - s); WEIGHTED: t = 0 squared error, 1 omega * squared
// error, 2 omega * |d|, 3 omega * (1 - s).  One fixed order within the workgroup.
template <bool WEIGHTED>
__device__ __forceinline__ void store_partials(const LossSums& a, double* __restrict__ partial, int slots, int slot, double* s4)
{
    constexpr int first = WEIGHTED ? 2 : 1; // the term of |d|
    const double t_sq = block_sum_256(a.sq, s4);
    double t_wsq = 0.0;
    if (WEIGHTED) t_wsq = block_sum_256(a.wsq, s4);
    const double t_l1 = block_sum_256(a.l1, s4), t_ds = block_sum_256(a.ds, s4);
    if (threadIdx.x == 0) {
        partial[slot] = t_sq;
        if (WEIGHTED) partial[(size_t)slots + slot] = t_wsq;
        partial[(size_t)first * slots + slot] = t_l1;
        partial[(size_t)(first + 1) * slots + slot] = t_ds;
    }
}

template <bool HALF, bool WEIGHTED>
__device__ __forceinline__ void loss_moments_body(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                  const float* __restrict__ omega, int W, int H, int tiles_x, const LossWindow& win,
                                                  float* __restrict__ maps, double* __restrict__ partial, int slots, int want_l1,
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

    LossSums a;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (px < W && py0 + k < H) {
            const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
            pixel_terms<WEIGHTED>(loss_load<HALF>(image0, i), loss_load<HALF>(image_ref, i), WEIGHTED ? omega[i] : 1.0f, want_l1 != 0, a);
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
                // derivatives of 1 - s with respect to mu_x (through the variances too), w*x^2 and w*xy; y is fixed
                const float mA = (2.0f * muy * (A1 - A2) + 2.0f * mux * s * (B2 - B1)) * invD;
                const float mB = s / B2;
                const float mC = -2.0f * A1 * invD;
                const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
                const float om = WEIGHTED ? omega[i] : 1.0f; // (read here, behind the window passes; the line is in the cache since the pixel terms)
                a.ds += WEIGHTED ? (double)om * (double)(1.0f - s) : (double)(1.0f - s);
                maps[(size_t)(c * 3 + 0) * plane + i] = under<WEIGHTED>(om, mA);
                maps[(size_t)(c * 3 + 1) * plane + i] = under<WEIGHTED>(om, mB);
                maps[(size_t)(c * 3 + 2) * plane + i] = under<WEIGHTED>(om, mC);
            }
        }
    }
    store_partials<WEIGHTED>(a, partial, slots, tile, red);
}

template <bool HALF, bool WEIGHTED>
__device__ __forceinline__ void loss_adjoint_body(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                  const float* __restrict__ omega, int W, int H, int tiles_x, const LossWindow& win,
                                                  const float* __restrict__ maps, float w_mse, float w_l1, float w_dssim,
                                                  float4* __restrict__ dimage, const DeviceStatus* __restrict__ status, int iteration)
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
            const size_t i = (size_t)(py0 + k) * (size_t)W + (size_t)px;
            const float om = WEIGHTED ? omega[i] : 1.0f; // the one read of the plane, behind everything else
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = chan(x[k], c) - chan(y[k], c);
                float v = w_dssim * g[k][c];
                if (w_mse > 0.0f) v += under<WEIGHTED>(om, w_mse * d);
                if (w_l1 > 0.0f) v += under<WEIGHTED>(om, w_l1 * sign0(d));
                o[c] = v;
            }
            dimage[i] = make_float4(o[0], o[1], o[2], 0.0f);
        }
    }
}

// With weights (1, 0, 0) and no plane a channel is 1.0f * (x - y): the subtraction of main.cpp:616 and nothing else.
template <bool HALF, bool WEIGHTED>
__device__ __forceinline__ void loss_pointwise_body(const void* __restrict__ image0, const void* __restrict__ image_ref,
                                                    const float* __restrict__ omega, size_t pixels, float w_mse, float w_l1,
                                                    float4* __restrict__ dimage, double* __restrict__ partial, int slots,
                                                    const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ double red[4];
    if (status->first_nonfinite_iter < iteration) return;
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    LossSums a;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t i = base + (size_t)k * 256;
        if (i < pixels) {
            const float4 x = loss_load<HALF>(image0, i), y = loss_load<HALF>(image_ref, i);
            const float om = WEIGHTED ? omega[i] : 1.0f;
            pixel_terms<WEIGHTED>(x, y, om, w_l1 > 0.0f, a);
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = chan(x, c) - chan(y, c);
                float v = 0.0f;
                if (w_mse > 0.0f) v = under<WEIGHTED>(om, w_mse * d);
                if (w_l1 > 0.0f) v = w_mse > 0.0f ? v + under<WEIGHTED>(om, w_l1 * sign0(d)) : under<WEIGHTED>(om, w_l1 * sign0(d));
                o[c] = v;
            }
            dimage[i] = make_float4(o[0], o[1], o[2], 0.0f);
        }
    }
    store_partials<WEIGHTED>(a, partial, slots, (int)blockIdx.x, red);
}

// The totals of the terms in `mask` (bit t = term t of TERMS), one workgroup, one fixed order: thread t adds slots t, t + 256,
// ..., then the block sum -- the pattern of sqerr_sum_small without its limit on the number of slots.  out: all TERMS totals.
// TERMS == kWeightedTerms: out3, the slot of the unweighted ring, receives terms 0, 2 and 3.
template <int TERMS>
__device__ __forceinline__ void loss_finalize_body(const double* __restrict__ partial, int slots, int count, int mask,
                                                   double* __restrict__ out, double* __restrict__ out3, double* __restrict__ sqerr_out,
                                                   const DeviceStatus* __restrict__ status, int iteration)
{
    __shared__ double s[4];
    if (status->first_nonfinite_iter < iteration) return;
    for (int t = 0; t < TERMS; t++) {
        if (!((mask >> t) & 1)) continue; // block-uniform
        double a = 0.0;
        for (int i = (int)threadIdx.x; i < count; i += 256) a += partial[(size_t)t * slots + i];
        const double total = block_sum_256(a, s);
        if (threadIdx.x == 0) {
            out[t] = total;
            if (TERMS == kWeightedTerms && t != 1) out3[t == 0 ? 0 : t - 1] = total;
            if (t == 0 && sqerr_out) *sqerr_out = total;
        }
    }
}

} // namespace s2d
