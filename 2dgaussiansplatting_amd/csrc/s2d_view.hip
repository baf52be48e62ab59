// s2d_view.hip -- view rendering: the record transform and the view raster kernel (s2d_view.h).
//
// view_raster_kernel is the forward walk (s2d_walk.h forward_tile, main.cpp:414-546) over the lists of a view's raster grid, with
// everything that serves training taken out: no hand-over to a backward walk, no retirement hint, no status word, no abort
// stamp, no counters.  The loop is its own; what it is made of is the walk's (s2d_walk.h): the staging of the lane masks
// (stage_masks), the body of a (pixel, entry) (blend_entry) and tile retirement (block_any_alive), operation for operation
// (-ffp-contract=off), which is what makes the identity view the bytes of image0.  One 256-thread workgroup per 16 x 16 tile of
// the grid, four wave64 of 8 x 8 pixels, lane = 8 * row + column.
//
// Without the hand-over a batch's masks and index words are dead behind its last barrier, so they need one copy instead of
// two and no index words at all: 5.1 KB of LDS per workgroup against the forward walk's 18.9 KB.
//
// Resolve: samples S per axis divide the tile edge and the grid is exactly out * S, so an S x S block of samples lies inside one
// wave's 8 x 8 block.  The lanes of a block exchange their colours (lane ^ 1, lane ^ 8; for S = 4 then lane ^ 2, lane ^ 16), the
// block's top-left lane forms ((p00 + p01) + (p10 + p11)) * 0.25f and stores the output pixel: no supersampled image exists in
// memory, and an RGBA8 view writes 4 bytes per output pixel.  Lane exchange rather than LDS: it runs once per tile behind a
// walk of hundreds of entries, needs no barrier and keeps the workgroup's LDS at the walk's.
//
// COVERAGE (S2D_CFG_COVERAGE): the walk blends through blend_entry_coverage, the coverage goes through the
// same resolve steps as the colours and ends in .w (RGBA8: the alpha byte, quantised like the colours).
#include "s2d_view.h"
#include "s2d_walk.h"

namespace s2d {

namespace {

// LDS of the view walk: per-entry record as the forward walk lays it out -- [0] pos.x, pos.y, a, b  [1] b, d, col_r, col_g
// [2] col_b, opacity, -, - -- and one copy of the lane masks.
struct ViewShared {
    float4 rec[B][3];
    unsigned long long mask[4 * B]; // [wave][entry]
    int4 alive;                     // per wave: does it still have a live pixel
};

} // namespace

__global__ __launch_bounds__(256) void view_transform_kernel(const float* __restrict__ splats, int n, ViewXform x,
                                                             float* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float in9[9], out9[9];
#pragma unroll
    for (int k = 0; k < 9; k++) in9[k] = splats[(size_t)i * 9 + k];
    view_row(x, in9, out9);
#pragma unroll
    for (int k = 0; k < 9; k++) out[(size_t)i * 9 + k] = out9[k];
}

template <bool EXACT, int S, bool RGBA8, bool COVERAGE = false>
__global__ __launch_bounds__(256) void view_raster_kernel(const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ list,
                                                          const ProjRec* __restrict__ proj, void* __restrict__ out, Geometry g,
                                                          int out_width)
{
    __shared__ ViewShared s;
    const int tile = (int)blockIdx.x;
    if (tile >= g.num_tiles) return;
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

    float cr = crg.x, cg = crg.y;
    if (S >= 2) {
        cr = resolve_level<1, 8>(cr);
        cg = resolve_level<1, 8>(cg);
        cb = resolve_level<1, 8>(cb);
        if constexpr (COVERAGE) ca = resolve_level<1, 8>(ca);
    }
    if (S == 4) {
        cr = resolve_level<2, 16>(cr);
        cg = resolve_level<2, 16>(cg);
        cb = resolve_level<2, 16>(cb);
        if constexpr (COVERAGE) ca = resolve_level<2, 16>(ca);
    }
    // the top-left sample of an output pixel stores it (S divides 8: lx % S == x % S); a block is inside the grid as a whole
    if (inside && (lx % S) == 0 && (ly % S) == 0) {
        const size_t o = (size_t)(y / S) * (size_t)out_width + (size_t)(x / S);
        if constexpr (COVERAGE) {
            if (RGBA8) reinterpret_cast<uint32_t*>(out)[o] = view_pack_rgba8(cr, cg, cb, ca);
            else reinterpret_cast<float4*>(out)[o] = make_float4(cr, cg, cb, ca);
        } else {
            if (RGBA8) reinterpret_cast<uint32_t*>(out)[o] = view_pack_rgba8(cr, cg, cb);
            else reinterpret_cast<float4*>(out)[o] = make_float4(cr, cg, cb, 1.0f); // .w reset, main.cpp:543-546
        }
    }
}

hipError_t launch_view_transform(const float* splats, int n, ViewXform x, float* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(view_transform_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, splats, n, x, out);
    return hipGetLastError();
}

namespace {

template <bool EXACT, int S>
void launch_view_format(const ViewRasterArgs& a, hipStream_t stream)
{
    const RasterArgs& w = a.walk;
    const dim3 grid((unsigned)w.g.num_tiles), block(256);
    if constexpr (!EXACT) { // (the coverage kernels exist with exp_approx alone: launch_view_raster)
        if (w.coverage) {
            if (a.rgba8)
                hipLaunchKernelGGL((view_raster_kernel<false, S, true, true>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.out, w.g, a.out_width);
            else
                hipLaunchKernelGGL((view_raster_kernel<false, S, false, true>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.out, w.g, a.out_width);
            return;
        }
    }
    if (a.rgba8)
        hipLaunchKernelGGL((view_raster_kernel<EXACT, S, true>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.out, w.g, a.out_width);
    else
        hipLaunchKernelGGL((view_raster_kernel<EXACT, S, false>), grid, block, 0, stream, w.tile_off, w.list, w.proj, a.out, w.g, a.out_width);
}

template <bool EXACT>
hipError_t launch_view_samples(const ViewRasterArgs& a, hipStream_t stream)
{
    switch (a.samples) {
    case 1: launch_view_format<EXACT, 1>(a, stream); break;
    case 2: launch_view_format<EXACT, 2>(a, stream); break;
    case 4: launch_view_format<EXACT, 4>(a, stream); break;
    default: return hipErrorInvalidValue; // a missing kernel is an error
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_view_raster(const ViewRasterArgs& a, hipStream_t stream)
{
    if (a.walk.g.num_tiles <= 0) return hipErrorInvalidValue;
    if (a.walk.coverage && a.walk.exact_exp) return hipErrorInvalidValue; // a missing kernel is an error
    return a.walk.exact_exp ? launch_view_samples<true>(a, stream) : launch_view_samples<false>(a, stream);
}

} // namespace s2d
