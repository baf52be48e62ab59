// s2d_raster_reference.hip -- reference-order validation mode (S2D_CFG_REFERENCE_ORDER): gradients and
// squared error bytes-equal to the reference's.  Three plain kernels.  Only order and per-term association differ from the fast
// path; the per-pixel decisions are the forward walk's, taken from its hand-over (exec_list, wave_masks) like
// raster_backward_kernel takes them.  No speed target: no LDS staging, one entry at a time.
#include "s2d_walk.h"

namespace s2d {

// One tile, one thread per pixel (the forward walk's pixel mapping, which the lane masks refer to).  For every entry the
// forward walk executed, in list order: the nine addends of main.cpp:619-704 (s2d_math.h reference_terms) into the pair's
// slot, exact +0 from the lanes the reference's loop body does not reach (not visited, main.cpp:595-598, or below the
// throughput cut-off, :604) -- adding +-0 to a chain that started at +0 never changes it.  Entries the walk did not
// execute have no reached pixel at all; their slots keep an older stamp.
__global__ __launch_bounds__(256) void reference_terms_kernel(const uint32_t* __restrict__ tile_off,
                                                              const uint32_t* __restrict__ exec_list,
                                                              const unsigned long long* __restrict__ wave_masks,
                                                              const uint32_t* __restrict__ tile_exec,
                                                              const ProjRec* __restrict__ proj,
                                                              const float4* __restrict__ image0,
                                                              const float4* __restrict__ src, RefOrder ro, Geometry g,
                                                              const DeviceStatus* __restrict__ status, int iteration, int exact,
                                                              int upstream)
{
    if (launch_is_void(status, 0, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    float4 fin = make_float4(0.f, 0.f, 0.f, 0.f), dL = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c.inside) {
        fin = image0[pixel_index(c, g)];                                 // finalColor, main.cpp:613
        const float4 s = src[pixel_index(c, g)];
        dL = upstream ? s : make_float4(fin.x - s.x, fin.y - s.y, fin.z - s.z, 0.0f); // main.cpp:616
        if (!upstream) {                                                 // main.cpp:801-802
            const float ex = dL.x * 255.0f, ey = dL.y * 255.0f, ez = dL.z * 255.0f;
            ro.pixel_sqerr[pixel_index(c, g)] = ex * ex + ey * ey + ez * ez;
        }
    }
    int lx, ly;
    pixel_of_thread(c.tid, &lx, &ly);
    const int at = ly * kTile + lx;
    RefPixel px = {0.0f, 0.0f, 0.0f, 1.0f};                              // image1 = (0,0,0,1), main.cpp:549
    const uint32_t beg = tile_off[tile], end = beg + tile_exec[tile];
    for (uint32_t e = beg; e < end; e++) {
        const uint32_t idx = exec_list[e];
        const unsigned long long wm = wave_masks[(size_t)e * 4 + c.w];
        float t[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (((wm >> c.lane) & 1ull) != 0ull && !(px.T < kMinThroughput)) {
            const ProjRec* r = proj + idx;
            const float4 q0 = r->q0, q1 = r->q1, q2 = r->q2, q3 = r->q3;
            const float* sp = ro.splats + (size_t)idx * 9;
            const RefSplat s = {q0.z, q0.w, q0.w, q1.x, q2.w, q3.x, sp[2], sp[3], q1.y, q1.z, q1.w, q2.x};
            float vx, vy;
            const float d2 = quad_form_at(c.pxy.x, c.pxy.y, q0.x, q0.y, s, &vx, &vy);
            const float G = exact ? expf_ref(-0.5f * d2) : gauss_from_d2(d2); // main.cpp:610, :51
            reference_terms(s, G, vx, vy, px, fin.x, fin.y, fin.z, dL.x, dL.y, dL.z, t);
        }
        const TileRect rc = ro.rects[idx];
        const uint32_t slot = ro.offsets[idx] + (uint32_t)(c.ty - g.trow0 - rc.ty0) * (uint32_t)(rc.tx1 - rc.tx0 + 1) + (uint32_t)(c.tx - rc.tx0);
        if (slot >= ro.capacity) continue; // (cannot happen while the lists are those of `rects`)
        float* dst = ro.terms + (size_t)slot * kRefTermsStride + at;
#pragma unroll
        for (int k = 0; k < 9; k++) dst[k * kTile * kTile] = t[k];
        if (c.tid == 0) ro.stamp[slot] = ro.now;
    }
}

// One thread per (splat, component): ONE fp32 chain from the value already in the gradient buffer (s2d_backward
// accumulates) through the splat's terms in the reference's order, main.cpp:576-598 -- pixel rows ascending, columns
// ascending, i.e. tile rows of its binned rectangle, pixel rows of a tile row, tiles left to right, their sixteen columns.
// Slots no pass stamped `now` (the tile never executed the entry) count as all zero.
__global__ __launch_bounds__(256) void reference_sum_kernel(RefOrder ro, float* __restrict__ grads, int need_opacity_grad,
                                                            const DeviceStatus* __restrict__ status, int iteration)
{
    if (launch_is_void(status, 0, iteration)) return;
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)ro.n * 9) return;
    const int i = (int)(q / 9), k = (int)(q - (long long)i * 9);
    if (k == 8 && !need_opacity_grad) return; // dSplats.opacity left as it is on request
    if (ro.counts[i] == 0u) return;
    const TileRect r = ro.rects[i];
    const uint32_t o = ro.offsets[i], wt = (uint32_t)(r.tx1 - r.tx0 + 1), ht = (uint32_t)(r.ty1 - r.ty0 + 1);
    float acc = grads[(size_t)i * 9 + k];
    for (uint32_t ty = 0; ty < ht; ty++) {
        const uint32_t row = o + ty * wt;
        if (row + wt > ro.capacity) break; // (as in reference_terms_kernel)
        bool any = false;
        for (uint32_t tx = 0; tx < wt; tx++) any = any || ro.stamp[row + tx] == ro.now;
        if (!any) continue;
        for (int py = 0; py < kTile; py++)
            for (uint32_t tx = 0; tx < wt; tx++) {
                if (ro.stamp[row + tx] != ro.now) continue;
                const float4* p = reinterpret_cast<const float4*>(ro.terms + (size_t)(row + tx) * kRefTermsStride + (k * kTile + py) * kTile);
                const float4 a = p[0], b = p[1], c = p[2], d = p[3];
                acc += a.x; acc += a.y; acc += a.z; acc += a.w;
                acc += b.x; acc += b.y; acc += b.z; acc += b.w;
                acc += c.x; acc += c.y; acc += c.z; acc += c.w;
                acc += d.x; acc += d.y; acc += d.z; acc += d.w;
            }
    }
    grads[(size_t)i * 9 + k] = acc;
}

// main.cpp:796-805: one double chain over the slab's pixels, row-major.  One wave: 256 values per round, four loads per
// lane in flight, then added lane by lane through v_readlane (the chain itself is sequential whatever is done).  Lanes
// past the end add +0.0, which leaves a chain of non-negative terms as it is.
__global__ __launch_bounds__(64) void reference_sqerr_kernel(const float* __restrict__ pixel_sqerr, size_t pixels,
                                                             double* __restrict__ out, const DeviceStatus* __restrict__ status,
                                                             int iteration)
{
    if (launch_is_void(status, 0, iteration)) return;
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (size_t base = 0; base < pixels; base += 256) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const size_t at = base + (size_t)j * 64 + lane;
            v[j] = at < pixels ? pixel_sqerr[at] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong((double)v[j]);
#pragma unroll
            for (int l = 0; l < 64; l++) acc += __longlong_as_double((long long)readlane_u64(bits, l));
        }
    }
    if (lane == 0) *out = acc;
}

hipError_t launch_reference_backward(const RasterArgs& a, const RefOrder& ro, hipStream_t stream)
{
    if (a.g.num_tiles <= 0) return hipSuccess;
    const bool up = a.upstream != nullptr;
    hipLaunchKernelGGL(reference_terms_kernel, dim3(raster_grid(a.g.num_tiles)), dim3(256), 0, stream, a.tile_off, a.exec_list,
                       a.wave_masks, a.tile_exec, a.proj, reinterpret_cast<const float4*>(a.image0),
                       up ? a.upstream : reinterpret_cast<const float4*>(a.image_ref), ro, a.g, a.status, a.iteration,
                       a.exact_exp ? 1 : 0, up ? 1 : 0);
    const long long chains = (long long)ro.n * 9;
    if (chains > 0) // (without splats the walk above still leaves every pixel's squared error)
        hipLaunchKernelGGL(reference_sum_kernel, dim3((unsigned)((chains + 255) / 256)), dim3(256), 0, stream, ro, a.grads,
                           a.need_opacity_grad ? 1 : 0, a.status, a.iteration);
    return hipGetLastError();
}

hipError_t launch_reference_sqerr(const float* pixel_sqerr, size_t pixels, double* out, const DeviceStatus* status, int iteration,
                                  hipStream_t stream)
{
    hipLaunchKernelGGL(reference_sqerr_kernel, dim3(1), dim3(64), 0, stream, pixel_sqerr, pixels, out, status, iteration);
    return hipGetLastError();
}

} // namespace s2d
