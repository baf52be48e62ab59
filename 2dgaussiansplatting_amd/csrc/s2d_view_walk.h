// s2d_view_walk.h -- what the view kernels are made of besides the shared walks (s2d_walk.h, s2d_walk_backward.h): the sample
// walk of a tile, the resolve of S x S samples to an output pixel with its store, and the adjoint of that resolve in lanes.
// Each has one definition here; view_raster_kernel (s2d_view.hip), backdrop_view_kernel (s2d_backdrop.hip),
// view_gradient_kernel (s2d_view_gradient.hip) and view_fit_kernel (s2d_view_fit.hip) are compositions of them, which is what
// keeps them the same operations in the same order (-ffp-contract=off): the identity view is the bytes of image0, the backdrop
// view is the composite per sample, s2d_step_view is the bytes of the view gradient from a target and an Adam step.
// DESIGN.md sections 17, 20, 24, 25.
//
// One 256-thread workgroup per 16 x 16 tile of the raster grid (out * S), four wave64 of 8 x 8 samples, lane = 8 * row + column.
// S divides the tile edge and the grid is exactly out * S, so an S x S block of samples lies inside one wave's 8 x 8 block, is
// inside the grid as a whole or not at all, and its top-left lane is the one that speaks for the output pixel.
#pragma once

#include "s2d_view.h"
#include "s2d_walk.h"

namespace s2d {

// LDS of the sample walk: per-entry record as the forward walk lays it out -- [0] pos.x, pos.y, a, b  [1] b, d, col_r, col_g
// [2] col_b, opacity, -, - -- and one copy of the lane masks.  Without a hand-over to a backward walk a batch's masks and index
// words are dead behind its last barrier, so they need one copy instead of two and no index words at all: 5.1 KB of LDS per
// workgroup against the forward walk's 18.9 KB.
struct ViewShared {
    float4 rec[B][3];
    unsigned long long mask[4 * B]; // [wave][entry]
    int4 alive;                     // per wave: does it still have a live pixel
};

// A sample of the raster grid when its walk has ended: where it is, and what the walk left.
struct ViewSample {
    int lx, ly, x, y; // inside the tile, inside the grid
    bool inside;
    float cr, cg, cb, ca, T; // main.cpp:414: (0,0,0,1) before the first entry; ca only with COVERAGE
};

// The sample walk of tile `tile`: the forward walk (s2d_walk.h forward_tile, main.cpp:414-546) with everything that serves
// training taken out -- no hand-over to a backward walk, no retirement hint, no status word, no abort stamp, no counters.  The
// loop is its own; what it is made of is the walk's: the staging of the lane masks (stage_masks), the body of a (pixel, entry)
// (blend_entry, with COVERAGE blend_entry_coverage) and tile retirement (block_any_alive), operation for operation.
template <bool EXACT, bool COVERAGE>
__device__ __forceinline__ ViewSample view_walk_tile(ViewShared& s, int tile, const uint32_t* __restrict__ tile_off,
                                                     const uint32_t* __restrict__ list, const ProjRec* __restrict__ proj, Geometry g)
{
    const int tx = tile % g.tiles_x, ty = tile / g.tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lx = (w % kWavesX) * kWaveW + (lane % kWaveW), ly = (w / kWavesX) * kWaveH + (lane / kWaveW); // pixel_of_thread
    const int x = tx * kTile + lx, y = ty * kTile + ly;
    const bool inside = x < g.W && y < g.row_end;
    const f2 pxy = mk2((float)x + 0.5f, (float)y + 0.5f); // pixel centre, main.cpp:523

    f2 crg = mk2(0.0f, 0.0f); // main.cpp:414: (0,0,0,1)
    float cb = 0.0f, T = 1.0f;
    [[maybe_unused]] float ca = 0.0f;
    unsigned long long alive_mask = __ballot(inside); // pixels still above the throughput cut-off (main.cpp:520), wave-uniform
    const uint32_t beg = tile_off[tile], end = tile_off[tile + 1];
    const int se = tid >> 2, sub = tid & 3;
    for (uint32_t base = beg; base < end; base += B) {
        const int cnt = (int)min((uint32_t)B, end - base);
        if (se < cnt) {
            const ProjRec* r = proj + list[base + se];
            const float4 q0 = r->q0, q1 = r->q1, q2 = r->q2;
            stage_masks(reinterpret_cast<uint32_t*>(s.mask), se, sub, q0, q1, __float_as_int(q2.y), __float_as_int(q2.z), ty * kTile,
                        tx * kTile, g.W, g.row_end);
            if (sub == 0) {
                s.rec[se][0] = q0;
                s.rec[se][1] = make_float4(q0.w, q1.x, q1.y, q1.z);
                s.rec[se][2] = make_float4(q1.w, q2.x, 0.0f, 0.0f);
            }
        }
        __syncthreads();
        if (alive_mask != 0ull) {
            const unsigned long long my_mask = (lane < cnt) ? s.mask[w * B + lane] : 0ull;
            // entries that touch a pixel of this wave's block that is still alive now; pixels only ever die, so nothing is
            // missed, and the per-entry test below still sees the mask of the moment
            unsigned long long cand = __ballot((my_mask & alive_mask) != 0ull);
            while (cand != 0ull) {
                const int e = __builtin_ctzll(cand);
                cand &= cand - 1ull;
                const unsigned long long act = readlane_u64(my_mask, e) & alive_mask; // visited (main.cpp:511-514), not cut off (:520)
                if (act == 0ull) continue;
                if constexpr (COVERAGE) {
                    const BlendedCoverage bl = blend_entry_coverage<EXACT>(s.rec[e][0], s.rec[e][1], s.rec[e][2], pxy, act, crg, cb, ca, T, alive_mask);
                    cb = bl.cb;
                    ca = bl.ca;
                    T = bl.T;
                    alive_mask = bl.alive_mask;
                } else {
                    const Blended bl = blend_entry<EXACT>(s.rec[e][0], s.rec[e][1], s.rec[e][2], pxy, act, crg, cb, T, alive_mask);
                    cb = bl.cb;
                    T = bl.T;
                    alive_mask = bl.alive_mask;
                }
            }
        }
        // (also the barrier behind which the next batch may overwrite the records and masks)
        if (!block_any_alive(&s.alive, w, lane, alive_mask)) break; // every pixel of the tile saturated: retire it
    }
    return ViewSample{lx, ly, x, y, inside, crg.x, crg.y, cb, ca, T};
}

// The resolve of one channel: S = 2 one level, S = 4 two.  Every lane runs it; the value is the output pixel's only in the
// top-left lane of its S x S block.
template <int S>
__device__ __forceinline__ float view_resolve(float v)
{
    static_assert(S == 1 || S == 2 || S == 4, "samples per axis");
    if (S >= 2) v = resolve_level<1, 8>(v);
    if (S == 4) v = resolve_level<2, 16>(v);
    return v;
}

// Resolve and store: the lanes of a block exchange their colours, the block's top-left lane stores the output pixel -- no
// supersampled image exists in memory, and an RGBA8 view writes 4 bytes per output pixel.  Lane exchange rather than LDS: it
// runs once per tile behind a walk of hundreds of entries, needs no barrier and keeps the workgroup's LDS at the walk's.
// COVERAGE: the coverage goes through the same resolve and ends in .w (RGBA8: the alpha byte, quantised like the colours).
template <int S, bool RGBA8, bool COVERAGE>
__device__ __forceinline__ void view_resolve_store(const ViewSample& p, void* __restrict__ out, int out_width)
{
    const float cr = view_resolve<S>(p.cr), cg = view_resolve<S>(p.cg), cb = view_resolve<S>(p.cb);
    [[maybe_unused]] float ca = 0.0f;
    if constexpr (COVERAGE) ca = view_resolve<S>(p.ca);
    // the top-left sample of an output pixel stores it (S divides 8: lx % S == x % S)
    if (p.inside && (p.lx % S) == 0 && (p.ly % S) == 0) {
        const size_t o = (size_t)(p.y / S) * (size_t)out_width + (size_t)(p.x / S);
        if constexpr (COVERAGE) {
            if (RGBA8) reinterpret_cast<uint32_t*>(out)[o] = view_pack_rgba8(cr, cg, cb, ca);
            else reinterpret_cast<float4*>(out)[o] = make_float4(cr, cg, cb, ca);
        } else {
            if (RGBA8) reinterpret_cast<uint32_t*>(out)[o] = view_pack_rgba8(cr, cg, cb);
            else reinterpret_cast<float4*>(out)[o] = make_float4(cr, cg, cb, 1.0f); // .w reset, main.cpp:543-546
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// The adjoint of the resolve, between forward_tile and backward_tile (view_gradient_kernel, view_fit_kernel).
// ---------------------------------------------------------------------------------------------------

// Is this thread the top-left sample of an output pixel, and which pixel (*o, valid for every sample of the grid)?
template <int S>
__device__ __forceinline__ bool view_top_lane(const TileCtx& c, int out_width, size_t* o)
{
    static_assert(S == 1 || S == 2 || S == 4, "samples per axis");
    int lx, ly;
    pixel_of_thread(c.tid, &lx, &ly);
    *o = (size_t)(c.y / S) * (size_t)out_width + (size_t)(c.x / S);
    return c.inside && (lx % S) == 0 && (ly % S) == 0;
}

// resolved - target in the top-left lane of an output pixel, zero in every other: the view's pixel as view_resolve_store forms
// it, then one fp32 subtraction per channel.
template <int S>
__device__ __forceinline__ float4 view_minus_target(const float4 fin, bool top, const float4* __restrict__ target, size_t o)
{
    const float rr = view_resolve<S>(fin.x), rg = view_resolve<S>(fin.y), rb = view_resolve<S>(fin.z);
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
    if (top) {
        const float4 t = target[o];
        u = make_float4(rr - t.x, rg - t.y, rb - t.z, 0.0f);
    }
    return u;
}

// The gradient of an output pixel, held by its top-left lane, to every sample of its block: each lane reads it from there
// (__shfl from lane & ~mask, mask = the lane bits of the block: 1 | 8, and for S = 4 also 2 | 16) and multiplies it by 0.25f
// once per level of the resolve -- exact, so a NumPy `repeat` times 0.25^levels gives the same bits.
template <int S>
__device__ __forceinline__ void view_broadcast(float4& u, int lane)
{
    if (S >= 2) {
        constexpr int kBlockBits = S == 4 ? (1 | 2 | 8 | 16) : (1 | 8);
        constexpr int kLevels = S == 4 ? 2 : 1;
        const int from = lane & ~kBlockBits;
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
}

// What backward_tile takes for a sample outside the grid: no final colour and no gradient.
__device__ __forceinline__ void view_zero_outside(const TileCtx& c, float4& fin, float4& u)
{
    if (!c.inside) {
        fin = make_float4(0.f, 0.f, 0.f, 0.f);
        u = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

} // namespace s2d
