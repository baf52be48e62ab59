// s2d_optim.hip -- init(), the Adam step with constraints and finite guard, and small utilities.
#include <hip/hip_fp16.h>

#include "s2d_device.h"
#include "s2d_adam.h"

namespace s2d {

// init(), main.cpp:280-305: one thread per splat; Adam state zeroed (main.cpp:285-286).
__global__ __launch_bounds__(256) void init_splats_kernel(float* __restrict__ splats, float* __restrict__ adams, int n,
                                                          int W, int H)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Splat s = init_splat((uint32_t)i, W, H);
    float* o = splats + (size_t)i * 9;
    o[0] = s.pos_x; o[1] = s.pos_y; o[2] = s.sx; o[3] = s.sy; o[4] = s.rot;
    o[5] = s.col_r; o[6] = s.col_g; o[7] = s.col_b; o[8] = s.opacity;
    float* a = adams + (size_t)i * 18;
#pragma unroll
    for (int k = 0; k < 18; k++) a[k] = 0.0f;
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ splats, float* __restrict__ adams,
                                                   float* __restrict__ grads, const uint32_t* __restrict__ held_ids,
                                                   const uint32_t* __restrict__ held_count, int n, Geometry g,
                                                   float beta1t, float beta2t, float lr, int mode, int iteration,
                                                   DeviceStatus* __restrict__ status, ProjRec* __restrict__ proj,
                                                   const TileRect* __restrict__ rects, int check_stamp,
                                                   int* __restrict__ host_stamp, uint8_t* __restrict__ dormant, SqerrJob sq,
                                                   int compact, int proj_current)
{
    __shared__ __attribute__((aligned(16))) float buf[256 * 18];
    __shared__ uint32_t s_idbuf[256];
    __shared__ uint64_t s_live_words[4];
    if (!adam_prologue(status, iteration, sq)) return;
    // (asked for here, beside the word the prologue has just read, and not where it is used: behind the gradients)
    const int last_failed_check = __hip_atomic_load(&status->rebin_needed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int total = held_ids ? (int)min(*held_count, (uint32_t)n) : n;
    const int base = blockIdx.x * 256, cnt = min(256, total - base), t = threadIdx.x;
    if (cnt <= 0) return;
    const bool mine = t < cnt;
    const uint32_t* s_ids = nullptr;
    int i = base + t;
    if (held_ids) { // only the splats this rank holds, from their compact list
        if (mine) {
            i = (int)held_ids[base + t];
            s_idbuf[t] = (uint32_t)i;
        }
        s_ids = s_idbuf;
        __syncthreads();
    }
    // compact: record base + t of `splats` / `adams` IS splat ids[t]'s (the rank's held splats in a compact array of their
    // own: whole lines, like the all-splats case); the gradient records stay where the raster kernels' atomics put them
    const uint32_t* const s_ids_state = compact ? nullptr : s_ids;
    float v[9], mv[18], gr[9];
    const bool asleep = mine && dormant != nullptr && dormant[i] != 0; // (in flight together with the gradients)
    // gradients in
    const uint32_t grads_nonzero = grads_fill(buf, grads, s_ids, base, cnt);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; k++) gr[k] = mine ? buf[t * 9 + k] : 0.0f;
    // A splat no live pixel sees receives a zero gradient; if its moments are zero as well (dormant[i]: they were after its
    // last full update, and nothing but this kernel has touched it since) the whole of main.cpp:721-750 leaves it exactly as
    // it is: m = v = 0, the step 0 / (0 + 1e-15), the clamps already applied.  Zero means +0, bit for bit, on both sides:
    // a first moment of -0.0 becomes +0 under a +0 gradient (0.9 * -0 + 0.1 * +0) and takes the sign of a -0.0 parameter
    // with it (-0 - -0 = +0), and a -0.0 gradient left in the buffer is not the +0 the reference starts its sums from
    // (main.cpp:550), so neither may be skipped over.  Such a splat is INERT in this launch: nothing of it is read beyond
    // the gradients just looked at and its dormant byte, nothing is written, and its projection record and containment
    // check stand as they are -- PROVIDED the record was made from these very parameters and the check was passed, which is
    // the context's Freshness::projection() (s2d_sequence.h) handed over as proj_current, with one addition the host cannot
    // see without waiting: the check before this one must not be a failed one that no list rebuild has answered yet
    // (rebuilds and checks share one sequence, so that is the stamp before ours), or a splat that failed it and went inert
    // would not fail this one.  Where the record is not known current every splat runs the step, which changes nothing
    // about an inert one but projects and checks it.  Splats are blended in index order, so the hidden ones are the later
    // ones -- 58 % of 10^6 on a 4096^2 image, nine in ten of them above index 440 000 -- but in runs between live ones: one
    // block in nine is made of them alone (profiles/r11).  Such a block returns here; any other moves the lines of its live
    // records only.
    const bool may_skip = proj == nullptr || (proj_current != 0 && last_failed_check != check_stamp - 1);
    bool live = false;
    if (mine) {
#pragma unroll
        for (int k = 0; k < 9; k++) live = live || (f32_bits(gr[k]) != 0u);
        if (!live) live = !may_skip || !asleep;
    }
    const uint64_t wave_live = __ballot(live);
    if ((t & 63) == 0) s_live_words[t >> 6] = wave_live;
    if (!__syncthreads_or(live)) return;
    const int inert_records = cnt - (__popcll(s_live_words[0]) + __popcll(s_live_words[1]) + __popcll(s_live_words[2]) + __popcll(s_live_words[3]));
    const uint64_t* const s_live = __builtin_amdgcn_readfirstlane(inert_records) == 0 ? nullptr : s_live_words;
    // zeros out, over the words that are not +0 already
    grads_rezero(grads, s_ids, base, cnt, grads_nonzero);
    // parameters in.  Every thread keeps its record's words, whichever of them were loaded: the copy is overwritten by the
    // moments below, and an inert record's words on a line it shares with a live one have to go back with that line.
    lds_fill<9>(buf, splats, s_ids_state, s_live, base, cnt);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = mine ? buf[t * 9 + k] : 0.0f;
    __syncthreads();
    // moments in
    lds_fill<18>(buf, adams, s_ids_state, s_live, base, cnt);
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 18; k++) mv[k] = buf[t * 18 + k];
        adam_update_one(v, mv, gr, g.W, g.H, beta1t, beta2t, lr, mode, iteration, status);
        if (dormant) { // all eighteen moments +0: the next +0 gradient changes nothing
            uint32_t any = 0u;
#pragma unroll
            for (int k = 0; k < 18; k++) any |= f32_bits(mv[k]);
            dormant[i] = any == 0u ? 1 : 0;
        }
        // moments out (each thread rewrites only its own record of the block's copy; the opacity slot goes back
        // unchanged when the checkbox is off)
#pragma unroll
        for (int k = 0; k < 18; k++) buf[t * 18 + k] = mv[k];
    }
    __syncthreads();
    lds_drain<18>(adams, buf, s_ids_state, s_live, base, cnt);
    __syncthreads();
    // parameters out
    if (mine) {
#pragma unroll
        for (int k = 0; k < 9; k++) buf[t * 9 + k] = v[k];
    }
    __syncthreads();
    lds_drain<9>(splats, buf, s_ids_state, s_live, base, cnt);
    if (proj && live) project_updated(v, i, g, status, proj, rects, check_stamp, host_stamp);
}

// ref(x,y) = (x/W, 1 - x/W, y/H, 1): main.cpp:261-267's commented generator plus a blue ramp.
__device__ __forceinline__ uint2 pack_half4(float4 c)
{
    const __half2 a = __floats2half2_rn(c.x, c.y), b = __floats2half2_rn(c.z, c.w);
    uint2 v;
    v.x = *reinterpret_cast<const uint32_t*>(&a);
    v.y = *reinterpret_cast<const uint32_t*>(&b);
    return v;
}

// image_ref holds rows [row_begin, row_end) of the image (the context's slab).
template <bool HALF>
__global__ __launch_bounds__(256) void synthetic_target_kernel(void* __restrict__ image_ref, int W, int H, int row_begin,
                                                               int row_end)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = row_begin + (int)blockIdx.y;
    if (x >= W || y >= row_end) return;
    const float fx = (float)x / (float)W;
    const float4 c = make_float4(fx, 1.0f - fx, (float)y / (float)H, 1.0f);
    const size_t at = (size_t)(y - row_begin) * W + x;
    if (HALF) reinterpret_cast<uint2*>(image_ref)[at] = pack_half4(c);
    else reinterpret_cast<float4*>(image_ref)[at] = c;
}

__global__ __launch_bounds__(256) void convert_f32_to_f16_kernel(const float4* __restrict__ src, uint2* __restrict__ dst,
                                                                 size_t pixels)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < pixels) dst[i] = pack_half4(src[i]);
}

__global__ __launch_bounds__(256) void convert_f16_to_f32_kernel(const uint2* __restrict__ src, float4* __restrict__ dst,
                                                                 size_t pixels)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    const uint2 v = src[i];
    const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&v.x));
    const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&v.y));
    dst[i] = make_float4(a.x, a.y, b.x, b.y);
}

__global__ __launch_bounds__(256) void test_sincos_kernel(const float* __restrict__ x, int n, float* __restrict__ s,
                                                          float* __restrict__ c)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    s[i] = sinf_ref(x[i]);
    c[i] = cosf_ref(x[i]);
}

hipError_t launch_init_splats(float* splats, float* adams, int n, int W, int H, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(init_splats_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, splats, adams, n, W, H);
    return hipGetLastError();
}

hipError_t launch_adam(const AdamArgs& a, hipStream_t stream)
{
    if (a.n <= 0) return hipSuccess;
    if (a.controls) return launch_adam_controls(a, stream); // (s2d_optim_controls.hip)
    hipLaunchKernelGGL(adam_kernel, dim3((a.n + 255) / 256), dim3(256), 0, stream, a.splats, a.adams, a.grads, a.held_ids,
                       a.held_count, a.n, a.g, a.beta1t, a.beta2t, a.lr, a.mode, a.iteration, a.check.status, a.proj,
                       (const TileRect*)a.check.rects, a.check.stamp, a.check.host_stamp, a.dormant, a.sq,
                       (a.compact && a.held_ids) ? 1 : 0, a.proj_current ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_synthetic_target(void* image_ref, bool half_images, int W, int H, int row_begin, int row_end, hipStream_t stream)
{
    const dim3 grid((W + 255) / 256, row_end - row_begin);
    if (half_images)
        hipLaunchKernelGGL(synthetic_target_kernel<true>, grid, dim3(256), 0, stream, image_ref, W, H, row_begin, row_end);
    else
        hipLaunchKernelGGL(synthetic_target_kernel<false>, grid, dim3(256), 0, stream, image_ref, W, H, row_begin, row_end);
    return hipGetLastError();
}

hipError_t launch_convert_f32_to_f16(const float4* src, void* dst, size_t pixels, hipStream_t stream)
{
    if (!pixels) return hipSuccess;
    hipLaunchKernelGGL(convert_f32_to_f16_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, src,
                       reinterpret_cast<uint2*>(dst), pixels);
    return hipGetLastError();
}

hipError_t launch_convert_f16_to_f32(const void* src, float4* dst, size_t pixels, hipStream_t stream)
{
    if (!pixels) return hipSuccess;
    hipLaunchKernelGGL(convert_f16_to_f32_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint2*>(src), dst, pixels);
    return hipGetLastError();
}

hipError_t launch_test_sincos(const float* x, int n, float* s, float* c, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(test_sincos_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, x, n, s, c);
    return hipGetLastError();
}

} // namespace s2d
