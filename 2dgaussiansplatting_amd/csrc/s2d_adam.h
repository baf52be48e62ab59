// s2d_adam.h -- what the two Adam kernels are made of (s2d_optim.hip: adam_kernel, the plain launch;
// s2d_optim_controls.hip: adam_controls_kernel, the launch under s2d_set_optim / s2d_set_frozen): the update of one splat,
// the projection of what it wrote, the launch's prologue, and the moves of a block's records through LDS.  Device code,
// included by those two units only.  (Two units: with both kernels in one, the compiler schedules the plain one differently,
// and that one is to stay instruction for instruction what it was -- DESIGN.md section 15.)
#pragma once

#include "s2d_device.h"

namespace s2d {

__device__ __forceinline__ bool finite_f32(float x) { return (f32_bits(x) & 0x7f800000u) != 0x7f800000u; }

// main.cpp:721-785 for one splat: the nine Adam updates, the constraints and the finite guard, on values held in
// registers.  The scalar order of Splat (pos.xy, sx, sy, rot, color.rgb, opacity) and of SplatAdam (pos[2], sx, sy, rot,
// color[3], opacity) is the same, so scalar k of the splat pairs with Adam slot k.  The nine updates are independent,
// so the reference's update order (color, pos, sx, sy, rot, opacity; main.cpp:723-738) does not matter.
// mode: bit 0 = optimizeOpacity (main.cpp:735-738), bit 1 = fp32 Adam quotient (S2D_CFG_ADAM_FP32).
__device__ __forceinline__ void adam_update_one(float (&v)[9], float (&mv)[18], const float (&gr)[9], int W, int H, float beta1t,
                                                float beta2t, float lr, int mode, int iteration, DeviceStatus* status)
{
#pragma unroll
    for (int k = 0; k < 9; k++)
        if (k < 8 || (mode & 1))
            v[k] = adam_optimize(mv[2 * k], mv[2 * k + 1], v[k], gr[k], lr, beta1t, beta2t, (mode & 2) != 0);
    // constraints, main.cpp:741-749
    v[0] = glm_clamp(v[0], 0.0f, (float)W - 1.0f);
    v[1] = glm_clamp(v[1], 0.0f, (float)H - 1.0f);
    v[2] = glm_clamp(v[2], 1.0f, 1024.0f);
    v[3] = glm_clamp(v[3], 1.0f, 1024.0f);
    v[5] = glm_clamp(v[5], 0.0f, 1.0f);
    v[6] = glm_clamp(v[6], 0.0f, 1.0f);
    v[7] = glm_clamp(v[7], 0.0f, 1.0f);
    v[8] = glm_clamp(v[8], 0.1f, 1.0f);
    // finite guard, main.cpp:752-785: color.xyz, sx, sy, rot, pos.x (pos.y and opacity are not checked)
    const bool ok = finite_f32(v[5]) && finite_f32(v[6]) && finite_f32(v[7]) && finite_f32(v[2]) &&
                    finite_f32(v[3]) && finite_f32(v[4]) && finite_f32(v[0]);
    if (!ok) {
        atomicOr(&status->nonfinite, 1);
        atomicMin(&status->first_nonfinite_iter, iteration);
    }
}

// The same with a rate per scalar: the nine of s2d_set_optim, resolved by the host for this iteration.  Each scalar is
// Adam::optimize (main.cpp:144-156) at its own alpha; constraints and finite guard as above.
__device__ __forceinline__ void adam_update_one(float (&v)[9], float (&mv)[18], const float (&gr)[9], int W, int H, float beta1t,
                                                float beta2t, const AdamRates& lr, int mode, int iteration, DeviceStatus* status)
{
#pragma unroll
    for (int k = 0; k < 9; k++)
        if (k < 8 || (mode & 1))
            v[k] = adam_optimize(mv[2 * k], mv[2 * k + 1], v[k], gr[k], lr.r[k], beta1t, beta2t, (mode & 2) != 0);
    // constraints, main.cpp:741-749
    v[0] = glm_clamp(v[0], 0.0f, (float)W - 1.0f);
    v[1] = glm_clamp(v[1], 0.0f, (float)H - 1.0f);
    v[2] = glm_clamp(v[2], 1.0f, 1024.0f);
    v[3] = glm_clamp(v[3], 1.0f, 1024.0f);
    v[5] = glm_clamp(v[5], 0.0f, 1.0f);
    v[6] = glm_clamp(v[6], 0.0f, 1.0f);
    v[7] = glm_clamp(v[7], 0.0f, 1.0f);
    v[8] = glm_clamp(v[8], 0.1f, 1.0f);
    // finite guard, main.cpp:752-785: color.xyz, sx, sy, rot, pos.x (pos.y and opacity are not checked)
    const bool ok = finite_f32(v[5]) && finite_f32(v[6]) && finite_f32(v[7]) && finite_f32(v[2]) &&
                    finite_f32(v[3]) && finite_f32(v[4]) && finite_f32(v[0]);
    if (!ok) {
        atomicOr(&status->nonfinite, 1);
        atomicMin(&status->first_nonfinite_iter, iteration);
    }
}

// Projection of the UPDATED splat for the next iteration's raster (main.cpp:423-436, 489-491) and the check against
// the rectangle its tile lists were built from, so that the next iteration needs no separate pass over the parameters.
__device__ __forceinline__ void project_updated(const float (&v)[9], int i, const Geometry& g, DeviceStatus* status,
                                                ProjRec* __restrict__ proj, const TileRect* __restrict__ rects,
                                                int check_stamp, int* __restrict__ host_stamp)
{
    // A rank that owns a row slab only ever reads the records of splats that can touch its rows.  A splat whose
    // 3-sigma circle (plus the 1-pixel skirt) stays clear of the slab has an empty exact rectangle, which every
    // binned rectangle covers: skip its projection (7/8 of the splats at 8 ranks).  NaNs fall through.
    const float reach = 3.0f * fmaxf(v[2], v[3]) + 2.0f;
    if (v[1] + reach < (float)g.row_begin || v[1] - reach > (float)g.row_end) {
        // ... but the re-used tile lists may still name it (it was inside when they were built, and one Adam step
        // can carry it out by any distance for a large training_rate or loaded moments): leave a record with
        // an empty row range (begY > endY) behind, so that the raster kernels see no footprint instead of its
        // stale one.
        proj[i].q2 = make_float4(v[8], as_f(1), as_f(0), 0.0f);
        return;
    }
    Splat s;
    s.pos_x = v[0]; s.pos_y = v[1]; s.sx = v[2]; s.sy = v[3]; s.rot = v[4];
    s.col_r = v[5]; s.col_g = v[6]; s.col_b = v[7]; s.opacity = v[8];
    const Projected p = project(s);
    proj[i] = pack_proj(p);
    if (!rect_still_covers(p, g, rects[i])) raise_rebin(status, check_stamp, host_stamp);
}

// The reference abort()s at the first non-finite parameter (main.cpp:752-785): later iterations do nothing.  (Strictly
// earlier: blocks of the detecting launch itself, which stores `iteration`, must all finish their work.)  Then the MSE of
// the iteration (main.cpp:796-805) from the tile errors the backward pass left, by the launch's first workgroups
// (block-uniform: all 256 threads take it together).  Returns false when the launch is to do nothing.
__device__ __forceinline__ bool adam_prologue(const DeviceStatus* status, int iteration, const SqerrJob& sq)
{
    if (status->first_nonfinite_iter < iteration) return false;
    if (sq.tile_sqerr != nullptr && blockIdx.x < (unsigned)kSqerrChunks)
        sqerr_reduce(sq.tile_sqerr, sq.num_tiles, sq.out, sq.scratch, (int)blockIdx.x, min((int)gridDim.x, kSqerrChunks));
    return true;
}

// Adam launch: one splat per thread, 256 records per block, every array moved through LDS so that global memory is
// accessed in runs of consecutive dwords instead of one record per lane.  (A thread reading its own 36-byte record
// dword by dword makes every load instruction touch 18 cache lines per wave, 36 for the 72-byte moments: the
// record-by-record form of this kernel ran at 1.8 TB/s, 192 us at 10^6 splats.)
//   * all splats in index order (ids == nullptr): a block's records are contiguous -- whole float4 lines;
//   * slab OWNERSHIP (s2d_halo.hip): the block walks 256 entries of the rank's compact, ascending list of held splats;
//     element e of the block's copy is dword e % w of record ids[e / w], so consecutive lanes still read consecutive
//     dwords of a record (and usually of neighbouring records).
// Also re-zeroes the gradient records (main.cpp:550 value-initialises dSplats every iteration).
//
// Parameters and moments move only where a LIVE record needs them (s_live: bit r of the block's 256 = record r runs the
// step): a 16-byte line is loaded and stored when one of the (at most two) records it holds words of is live, and the
// words of an inert neighbour on such a line go back as they came.  s_live == nullptr: every record of the block is live
// (small scenes, where nothing is hidden: the arrays move as whole lines without a look at the masks).
__device__ __forceinline__ bool record_live(const uint64_t* s_live, int r)
{
    return s_live == nullptr || ((s_live[r >> 6] >> (r & 63)) & 1ull) != 0ull;
}

template <int WIDTH>
__device__ __forceinline__ bool line_live(const uint64_t* s_live, int q) // WIDTH >= 4: words 4q .. 4q + 3 lie in two records at most
{
    return s_live == nullptr || record_live(s_live, (4 * q) / WIDTH) || record_live(s_live, (4 * q + 3) / WIDTH);
}

template <int WIDTH>
__device__ __forceinline__ void lds_fill(float* lds, const float* __restrict__ src, const uint32_t* s_ids, const uint64_t* s_live,
                                         int base, int cnt)
{
    const int floats = cnt * WIDTH;
    if (s_ids == nullptr) { // contiguous and 16-byte aligned: a block starts at a multiple of 256 records
        const float* p = src + (size_t)base * WIDTH;
        const int vec = floats >> 2;
        // every load of the thread asked for before the first is waited for: one memory round trip, not one per line (a
        // launch of a few workgroups lasts as long as one block's chain of them)
        constexpr int kLines = (256 * WIDTH / 4 + 255) / 256;
        float4 x[kLines];
        uint32_t take = 0u;
#pragma unroll
        for (int j = 0; j < kLines; j++) {
            const int q = (int)threadIdx.x + 256 * j;
            take |= (q < vec && line_live<WIDTH>(s_live, q) ? 1u : 0u) << j;
        }
#pragma unroll
        for (int j = 0; j < kLines; j++) {
            x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((take >> j) & 1u) x[j] = reinterpret_cast<const float4*>(p)[(int)threadIdx.x + 256 * j];
        }
#pragma unroll
        for (int j = 0; j < kLines; j++)
            if ((take >> j) & 1u) reinterpret_cast<float4*>(lds)[(int)threadIdx.x + 256 * j] = x[j];
        for (int q = (vec << 2) + threadIdx.x; q < floats; q += 256)
            if (record_live(s_live, q / WIDTH)) lds[q] = p[q];
    } else {
        for (int q = threadIdx.x; q < floats; q += 256)
            if (record_live(s_live, q / WIDTH)) lds[q] = src[(size_t)s_ids[q / WIDTH] * WIDTH + q % WIDTH];
    }
}

template <int WIDTH>
__device__ __forceinline__ void lds_drain(float* __restrict__ dst, const float* lds, const uint32_t* s_ids, const uint64_t* s_live,
                                          int base, int cnt)
{
    const int floats = cnt * WIDTH;
    if (s_ids == nullptr) {
        float* p = dst + (size_t)base * WIDTH;
        const int vec = floats >> 2;
        for (int q = threadIdx.x; q < vec; q += 256)
            if (line_live<WIDTH>(s_live, q)) reinterpret_cast<float4*>(p)[q] = reinterpret_cast<const float4*>(lds)[q];
        for (int q = (vec << 2) + threadIdx.x; q < floats; q += 256)
            if (record_live(s_live, q / WIDTH)) p[q] = lds[q];
    } else {
        for (int q = threadIdx.x; q < floats; q += 256)
            if (record_live(s_live, q / WIDTH)) dst[(size_t)s_ids[q / WIDTH] * WIDTH + q % WIDTH] = lds[q];
    }
}

// The block's gradient records into LDS, all of them: whether a record is live is read off them.  Returns which of the
// thread's loads (bit j: its j-th) brought a word that is not +0 -- the only ones grads_rezero has to store over.
__device__ __forceinline__ uint32_t grads_fill(float* lds, const float* __restrict__ grads, const uint32_t* s_ids, int base, int cnt)
{
    const int floats = cnt * 9;
    uint32_t nz = 0u;
    int j = 0;
    if (s_ids == nullptr) {
        const float* p = grads + (size_t)base * 9;
        const int vec = floats >> 2;
        for (int q = threadIdx.x; q < vec; q += 256, j++) {
            const float4 x = reinterpret_cast<const float4*>(p)[q];
            reinterpret_cast<float4*>(lds)[q] = x;
            nz |= ((f32_bits(x.x) | f32_bits(x.y) | f32_bits(x.z) | f32_bits(x.w)) != 0u ? 1u : 0u) << j;
        }
        for (int q = (vec << 2) + threadIdx.x; q < floats; q += 256, j++) {
            const float x = p[q];
            lds[q] = x;
            nz |= (f32_bits(x) != 0u ? 1u : 0u) << j;
        }
    } else {
        for (int q = threadIdx.x; q < floats; q += 256, j++) {
            const float x = grads[(size_t)s_ids[q / 9] * 9 + q % 9];
            lds[q] = x;
            nz |= (f32_bits(x) != 0u ? 1u : 0u) << j;
        }
    }
    return nz;
}

__device__ __forceinline__ void grads_rezero(float* __restrict__ grads, const uint32_t* s_ids, int base, int cnt, uint32_t nz)
{
    const int floats = cnt * 9;
    int j = 0;
    if (s_ids == nullptr) {
        float* p = grads + (size_t)base * 9;
        const int vec = floats >> 2;
        for (int q = threadIdx.x; q < vec; q += 256, j++)
            if ((nz >> j) & 1u) reinterpret_cast<float4*>(p)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = (vec << 2) + threadIdx.x; q < floats; q += 256, j++)
            if ((nz >> j) & 1u) p[q] = 0.0f;
    } else {
        for (int q = threadIdx.x; q < floats; q += 256, j++)
            if ((nz >> j) & 1u) grads[(size_t)s_ids[q / 9] * 9 + q % 9] = 0.0f;
    }
}

} // namespace s2d
