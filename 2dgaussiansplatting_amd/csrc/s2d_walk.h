// s2d_walk.h -- what every walk over a tile's splat list is made of: the tile / wave / pixel mapping, fp32 pairs, the staging
// of the lane masks, tile retirement, the forward walk itself (forward_tile) and the flag-to-template dispatch of the launchers.
// Included by every raster unit (s2d_raster*.hip) and by the view (s2d_view.hip); device code, hipcc only.
#pragma once
#include <hip/hip_fp16.h>
#include <type_traits>

#include "s2d_device.h"

namespace s2d {

constexpr int B = kRasterBatch;
static_assert(B == 64, "lane l of a wave holds the mask of batch entry l");

// Forward batch sizes from where the tile retired in the previous launch (retire_hint[tile]: list position, relative to the
// tile's first, one past the last executed entry; kNoHint: unknown, or the walk ran to the end of its list).  A tile that
// retires has otherwise staged half a batch too many, four row solves per staging thread each.  Up to the hint batches are
// full; the batch the hint falls into ends at it, rounded up to a staging wave's 16 entries (the other waves go straight
// to the barrier); a tile that lives longer than last time goes on in batches of kHintFollow.  It is a hint and nothing
// else: every pixel still sees every entry of its list in order until the tile retires, whatever the word holds -- also
// one left by other lists or other splats, which is why nothing but the walk itself ever writes it.  Measured on top of
// the compacted hand-over, 4096^2 / 1 M (profiles/r06/ab_exec_handover.txt): slack behind the hint 0 / 4 / 8 / 16 entries
// +2.3 / +2.1 / +1.8 / +1.0 %, follow-up batches of 16 and 32 the same, and a hint kept across a list rebuild +0.3 % over
// one reset there.
constexpr uint32_t kNoHint = 0xFFFFFFFFu;
constexpr uint32_t kHintFollow = 16;

constexpr int kWaveW = 8;              // pixel columns per wave block (8x8 blocks: measured better than 16x4 strips,
constexpr int kWaveH = 64 / kWaveW;    // profiles/r01: 34 vs 37 executed entries per wave, 36 vs 33 active lanes)
constexpr int kWavesX = kTile / kWaveW;

// Block -> tile: dispatch order.  (An XCD-contiguous remap and a longest-list-first order were measured slower,
// profiles/r01/README.md: these kernels are VALU-issue-bound, not L2-bound.)
__device__ __forceinline__ int tile_of_block(int bid, const Geometry& g) { return bid < g.num_tiles ? bid : -1; }

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int src_lane)
{
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src_lane);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src_lane);
    return ((unsigned long long)hi << 32) | lo;
}

// Framebuffer / target pixel in HBM: RGBA32F (the reference's Image2DRGBA32, 16 B) or, with S2D_CFG_FP16_IMAGES,
// four IEEE halves (8 B, round-to-nearest-even on store).  Arithmetic is fp32 either way.
template <bool HALF>
__device__ __forceinline__ float4 load_pixel(const void* base, size_t i)
{
    if (HALF) {
        const uint2 v = reinterpret_cast<const uint2*>(base)[i];
        const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&v.x));
        const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&v.y));
        return make_float4(a.x, a.y, b.x, b.y);
    }
    return reinterpret_cast<const float4*>(base)[i];
}

template <bool HALF>
__device__ __forceinline__ void store_pixel(void* base, size_t i, float4 c)
{
    if (HALF) {
        const __half2 a = __floats2half2_rn(c.x, c.y), b = __floats2half2_rn(c.z, c.w);
        uint2 v;
        v.x = *reinterpret_cast<const uint32_t*>(&a);
        v.y = *reinterpret_cast<const uint32_t*>(&b);
        reinterpret_cast<uint2*>(base)[i] = v;
    } else {
        reinterpret_cast<float4*>(base)[i] = c;
    }
}

// A pair of fp32 values -- (vx,vy), (mx,my), the (r,g) colour channels, the two covariance dot products.  The blend
// and gradient arithmetic below is written on such pairs with every product and sum in the reference's order.
// A plain struct whose operators are two scalar VALU instructions each: on gfx950 a v_pk_{mul,add,fma}_f32 occupies a
// SIMD for ~4.3 cycles, a v_{mul,add,fma}_f32 for ~2.4 (tools/microbench/valu_rates.hip, profiles/r01/valu_rates.txt),
// so packed fp32 buys nothing and the register-pair assembly it needs costs (395 vs 413 it/s, profiles/r01/v8_*);
// the build passes -fno-slp-vectorize so LLVM does not re-pack these.
struct f2 {
    float x, y;
};
__device__ __forceinline__ f2 operator+(f2 a, f2 b) { return f2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ f2 operator-(f2 a, f2 b) { return f2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ f2 operator*(f2 a, f2 b) { return f2{a.x * b.x, a.y * b.y}; }
__device__ __forceinline__ f2 operator*(f2 a, float b) { return f2{a.x * b, a.y * b}; }
__device__ __forceinline__ f2 operator*(float a, f2 b) { return f2{a * b.x, a * b.y}; }
__device__ __forceinline__ f2 operator-(f2 a) { return f2{-a.x, -a.y}; }
__device__ __forceinline__ f2& operator+=(f2& a, f2 b) { a = a + b; return a; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return f2{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)}; }
__device__ __forceinline__ f2 mk2(float a, float b)
{
    f2 r;
    r.x = a;
    r.y = b;
    return r;
}

// Diagnostic counters (S2D_CFG_COUNT_PAIRS): a per-lane count is summed over the wave first and added by one lane (the build
// switches LLVM's atomic optimizer off, _build.py: nothing does this behind our back any more).
__device__ __forceinline__ void count_add(unsigned long long* counter, unsigned long long v, int lane)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if (lane == 0) atomicAdd(counter, v);
}

// Pixel of thread tid inside the tile.
__device__ __forceinline__ void pixel_of_thread(int tid, int* lx, int* ly)
{
    const int w = tid >> 6, lane = tid & 63;
    *lx = (w % kWavesX) * kWaveW + (lane % kWaveW);
    *ly = (w / kWavesX) * kWaveH + (lane / kWaveW);
}

// Staging thread (se = entry, sub = 0..3) evaluates tile rows sub*4 .. sub*4+3 of entry se and deposits the
// bits into the per-(wave, entry) lane masks, laid out s_mask[wave][entry] as 2 x 32-bit words each.
__device__ __forceinline__ int stage_masks(uint32_t* s_mask32, int se, int sub, const float4& q0, const float4& q1,
                                            int begY, int endY, int y_tile, int x_tile, int W, int row_end)
{
    uint32_t rm[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int yy = y_tile + sub * 4 + k;
        rm[k] = 0;
        if (yy < row_end) rm[k] = row_mask16(q0.x, q0.y, q0.z, q0.w, q1.x, begY, endY, yy, x_tile, W);
    }
    // waves (wy, 0) and (wy, 1) with wy = sub >> 1; rows (sub & 1) * 4 + k of the 8x8 block; lane = 8 * row + column
    const int wy = sub >> 1, half = sub & 1;
#pragma unroll
    for (int wx = 0; wx < 2; wx++) {
        const int sh = 8 * wx;
        const uint32_t word = ((rm[0] >> sh) & 0xFFu) | (((rm[1] >> sh) & 0xFFu) << 8) |
                              (((rm[2] >> sh) & 0xFFu) << 16) | (((rm[3] >> sh) & 0xFFu) << 24);
        s_mask32[((wy * 2 + wx) * B + se) * 2 + half] = word;
    }
    return (rm[0] != 0u) + (rm[1] != 0u) + (rm[2] != 0u) + (rm[3] != 0u); // non-empty rows (diagnostic counter)
}

// ---------------------------------------------------------------------------------------------------
// forward, main.cpp:414-546
// ---------------------------------------------------------------------------------------------------
// EXACT (S2D_CFG_EXACT_EXP): G = expf(-d2/2) instead of exp_approx -- the switch the reference keeps at main.cpp:51
// "for numerical varidation": the analytic gradients are those of the TRUE exponential, so only in this mode is the
// backward pass the derivative of the forward pass (tests/test_fd_end_to_end.py checks exactly that by finite differences).
// The expf is the one with the bits of the oracle's libm (s2d_math.h expf_ref), in every kernel of the mode: the device
// library's is accurate to 1 ulp but not equal to it, and a framebuffer that is an ulp off the reference's cannot be held
// to it on bits (tests/test_gpu_raster_variants.py does, for every exact variant).
template <bool EXACT>
__device__ __forceinline__ float gauss_of(float d2, bool* nonzero)
{
    if (EXACT) {
        *nonzero = true;
        return expf_ref(-0.5f * d2); // main.cpp:51, :527
    }
    return gauss_pow8(d2, nonzero);
}

// What a thread needs to know about its pixel and its place in the workgroup.
struct TileCtx {
    int tile, tx, ty;   // tile index (local to the slab), tile column, GLOBAL tile row
    int tid, lane, w;   // thread, lane, wave within the workgroup
    int x, y;           // pixel
    bool inside;        // pixel inside the image and the slab
    f2 pxy;             // pixel centre, main.cpp:523
};

__device__ __forceinline__ TileCtx tile_ctx(int tile, const Geometry& g)
{
    TileCtx c;
    c.tile = tile;
    c.tx = tile % g.tiles_x;
    c.ty = tile / g.tiles_x + g.trow0;
    c.tid = threadIdx.x;
    c.lane = c.tid & 63;
    c.w = c.tid >> 6;
    int lx, ly;
    pixel_of_thread(c.tid, &lx, &ly);
    c.x = c.tx * kTile + lx;
    c.y = c.ty * kTile + ly;
    c.inside = c.x < g.W && c.y < g.row_end;
    c.pxy = mk2((float)c.x + 0.5f, (float)c.y + 0.5f);
    return c;
}

// Where the thread's pixel sits in image0 / imageRef: the context stores only the rows of its slab.
__device__ __forceinline__ size_t pixel_index(const TileCtx& c, const Geometry& g) { return (size_t)(c.y - g.row_begin) * g.W + c.x; }

// LDS of the forward walk: per-entry record, three 16-B rows at one LDS address (one address register for the blend
// loop's reads):  [0] pos.x, pos.y, a, b   [1] b, d, col_r, col_g   [2] col_b, opacity, -, -
// (b twice: (a,b) and (b,d) are the two columns of inv_cov)
// mask and idx (the list word) in two copies, by batch parity: the hand-over to the backward walk reads them behind the
// last barrier of the batch, while fast threads already stage the next one.
struct FwdShared {
    float4 rec[B][3];
    unsigned long long mask[2][4 * B]; // [parity][wave][entry]
    uint32_t idx[2][B];
    unsigned long long touched[4];     // per wave: bit e = the body of entry e ran (posted with the alive flag)
    int4 alive;                        // per wave: does it still have a live pixel (block_any_alive)
};

// "Does any wave of the workgroup still have a live pixel?"  The answer of a wave is already uniform (its alive mask
// sits in scalar registers), so one lane posts it and everybody reads the four flags after the barrier --
// __syncthreads_or would first reduce the flag over the 64 lanes with eight DPP steps.  The flags are rewritten only
// behind the next batch's staging barrier.
__device__ __forceinline__ bool block_any_alive(int4* flags, int w, int lane, unsigned long long alive_mask)
{
    if (lane == 0) reinterpret_cast<int*>(flags)[w] = alive_mask != 0ull ? 1 : 0;
    __syncthreads();
    const int4 f = *flags;
    return ((f.x | f.y) | (f.z | f.w)) != 0;
}

// The same exchange at the end of a forward batch, which also carries the entries each wave executed: *exec_mask = bit e
// set <=> the body of entry e ran in at least one wave (uniform, in scalar registers).
__device__ __forceinline__ bool block_any_alive_exec(int4* flags, unsigned long long* touched4, int w, int lane,
                                                     unsigned long long alive_mask, unsigned long long touched,
                                                     unsigned long long* exec_mask)
{
    if (lane == 0) {
        reinterpret_cast<int*>(flags)[w] = alive_mask != 0ull ? 1 : 0;
        touched4[w] = touched;
    }
    __syncthreads();
    const int4 f = *flags;
    const unsigned long long m = (touched4[0] | touched4[1]) | (touched4[2] | touched4[3]);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)m), hi = __builtin_amdgcn_readfirstlane((uint32_t)(m >> 32));
    *exec_mask = ((unsigned long long)hi << 32) | lo;
    return ((f.x | f.y) | (f.z | f.w)) != 0;
}

// The forward body of one (pixel, entry), main.cpp:523-533, for the lanes of `act` (visited, main.cpp:511-514, and not cut off,
// :520), and the alive mask for the next entry.  Branch-free: lanes outside `act` run the same instructions with alpha forced
// to 0, which makes c += (T*c)*0 and T *= 1 exact no-ops.  The scalar mask itself is the select predicate.
// q0, q1, q2: the entry's record as FwdShared lays it out.  The training walks and the view (s2d_view.hip) blend through this one
// function, which is what makes the identity view the bytes of image0.
// (The colour pair by reference, the scalars by value and back in the result, on purpose: that is how the variables were
// used while the body stood in the loops -- crg through operator+=, the others directly -- and every kernel comes out of the
// compiler as it did then.  With the scalars by reference too, the register numbering of 38 kernels changes)
struct Blended {
    float cb, T;
    unsigned long long alive_mask;
};
template <bool EXACT>
__device__ __forceinline__ Blended blend_entry(const float4 q0, const float4 q1, const float4 q2, const f2 pxy, unsigned long long act,
                                               f2& crg, float cb, float T, unsigned long long alive_mask)
{
    const f2 v = pxy - mk2(q0.x, q0.y);                          // main.cpp:523-524
    const f2 m = mk2(q0.z, q0.w) * v.x + mk2(q1.x, q1.y) * v.y;  // inv_cov * v: (a vx + b vy, b vx + d vy)
    const f2 vm = v * m;
    bool nonzero;
    const float G = gauss_of<EXACT>(vm.x + vm.y, &nonzero);      // main.cpp:526-527
    const unsigned long long on = act & __ballot(nonzero);
    const float alpha = __builtin_amdgcn_inverse_ballot_w64(on) ? G * q2.y : 0.0f;
    crg += (T * mk2(q1.z, q1.w)) * alpha;                        // main.cpp:529-530: (T*c)*alpha
    cb += T * q2.x * alpha;                                      // main.cpp:531
    T *= (1.0f - alpha);                                         // main.cpp:533
    alive_mask &= __ballot(!(T < kMinThroughput));               // main.cpp:520, for the next splat
    return Blended{cb, T, alive_mask};
}

// The same body with the coverage channel (S2D_CFG_COVERAGE): ca += T * alpha, the colour sum of a channel
// whose colour is 1 in every splat ((T * 1) * alpha, the product of main.cpp:529-531 with c = 1) -- two more VALU operations per
// executed (wave, entry).  A function of its own, so that blend_entry and every kernel made of it stay what they were.
struct BlendedCoverage {
    float cb, ca, T;
    unsigned long long alive_mask;
};
template <bool EXACT>
__device__ __forceinline__ BlendedCoverage blend_entry_coverage(const float4 q0, const float4 q1, const float4 q2, const f2 pxy,
                                                                unsigned long long act, f2& crg, float cb, float ca, float T,
                                                                unsigned long long alive_mask)
{
    const f2 v = pxy - mk2(q0.x, q0.y);                          // main.cpp:523-524
    const f2 m = mk2(q0.z, q0.w) * v.x + mk2(q1.x, q1.y) * v.y;  // inv_cov * v: (a vx + b vy, b vx + d vy)
    const f2 vm = v * m;
    bool nonzero;
    const float G = gauss_of<EXACT>(vm.x + vm.y, &nonzero);      // main.cpp:526-527
    const unsigned long long on = act & __ballot(nonzero);
    const float alpha = __builtin_amdgcn_inverse_ballot_w64(on) ? G * q2.y : 0.0f;
    crg += (T * mk2(q1.z, q1.w)) * alpha;                        // main.cpp:529-530: (T*c)*alpha
    cb += T * q2.x * alpha;                                      // main.cpp:531
    ca += T * alpha;                                             // the same with c = 1
    T *= (1.0f - alpha);                                         // main.cpp:533
    alive_mask &= __ballot(!(T < kMinThroughput));               // main.cpp:520, for the next splat
    return BlendedCoverage{cb, ca, T, alive_mask};
}

// One tile's forward walk (main.cpp:419-536 for its pixels): leaves the final colour of this thread's pixel in
// (crg, cb) and hands the entries the backward walk has to run over to it.  The backward walk makes exactly this walk's
// per-pixel decisions, so the (wave, entry) bodies it will run are the ones that ran here: entry k (k = 0 ..) of them
// leaves its splat index in exec_list[beg + k] and its four lane masks in wave_masks[(beg + k) * 4 ..], beg = the
// tile's first list position; their number is returned.  Compacted positions never run ahead of list positions and
// [beg, end) belongs to this tile alone.  A counting walk (COUNT, whose statistics are defined on staged entries) hands
// over every staged entry at its list position instead, and the backward walk reads the list.
// CHUNK (scenes whose (tile, splat) pairs do not fit one set of lists, s2d_sequence.hip chunked_forward / chunked_backward): the
// list holds the
// splats of one INDEX RANGE only; the walk continues from the pixel's state after the ranges before it -- (crg, cb) and
// *T_io on entry -- and leaves the state for the range after it.  The reference's loop is front to back in index order
// (main.cpp:419), so cutting it at any index and carrying (colour, T) across the cut changes no operation.
// COVERAGE (s2d_raster_coverage.hip): the walk blends through blend_entry_coverage and leaves the pixel's coverage in *ca_out.
// THROUGHPUT (s2d_backdrop.hip): the plain walk, retirement hint included, that also leaves the pixel's final T in *T_io.
template <bool COUNT, bool EXACT, bool CHUNK = false, bool COVERAGE = false, bool THROUGHPUT = false>
__device__ __forceinline__ uint32_t forward_tile(FwdShared& s, const TileCtx& c, const uint32_t* __restrict__ tile_off,
                                             const uint32_t* __restrict__ list, const ProjRec* __restrict__ proj,
                                             unsigned long long* __restrict__ wave_masks, uint32_t* __restrict__ exec_list,
                                             uint32_t* __restrict__ retire_hint, const Geometry& g,
                                             PairCounters* __restrict__ counters, f2& crg, float& cb, float* T_io = nullptr,
                                             float* ca_out = nullptr)
{
    static_assert(!(COVERAGE && (COUNT || EXACT || CHUNK)), "the coverage channel: plain lists, exp_approx, no pair counting");
    static_assert(!(THROUGHPUT && (COUNT || EXACT || CHUNK || COVERAGE)), "the final throughput: plain lists, exp_approx, no pair counting");
    constexpr bool HINT = !COUNT && !CHUNK;
    const int tid = c.tid, lane = c.lane, w = c.w;
    const f2 pxy = c.pxy;
    float T = 1.0f;
    if (CHUNK) {
        T = *T_io;
    } else {
        crg = mk2(0.0f, 0.0f);                              // main.cpp:414: (0,0,0,1)
        cb = 0.0f;
    }
    [[maybe_unused]] float ca = 0.0f;
    // Pixels still above the throughput cut-off (main.cpp:520), as ONE wave-uniform 64-bit mask in scalar registers.
    // (A per-lane bool here costs ~15 scalar instructions per blended entry to merge with exec, and the CU's
    // single scalar unit -- not the SIMDs -- then bounds the loop; measured, profiles/r01/valu_rates.txt.)
    unsigned long long alive_mask = __ballot(CHUNK ? c.inside && !(T < kMinThroughput) : c.inside);
    unsigned long long n_vis = 0, n_act = 0, n_staged = 0, n_exec = 0, n_rows_hit = 0, n_staged_hit = 0;

    const uint32_t beg = tile_off[c.tile], end = tile_off[c.tile + 1];
    const int se = tid >> 2, sub = tid & 3;
    uint32_t n_out = 0; // entries handed over so far
    uint32_t hint = kNoHint, last_exec = 0;
    bool retired = false;
    if constexpr (HINT) hint = retire_hint[c.tile];
    int pb = 1;
    for (uint32_t base = beg, cnt_u = 0; base < end; base += cnt_u) {
        uint32_t want = B;
        if constexpr (HINT) {
            const uint32_t pos = base - beg;
            if (hint != kNoHint) {
                if (hint <= pos) want = kHintFollow;
                else if (hint - pos <= (uint32_t)B) want = (hint - pos + 15u) & ~15u;
            }
        }
        cnt_u = min(want, end - base);
        const int cnt = (int)cnt_u;
        pb ^= 1;
        unsigned long long* const s_mask = s.mask[pb];
        if (se < cnt) {
            const uint32_t idx = list[base + se];
            const ProjRec* r = proj + idx;
            const float4 q0 = r->q0, q1 = r->q1, q2 = r->q2;
            const int rows_hit = stage_masks(reinterpret_cast<uint32_t*>(s_mask), se, sub, q0, q1, __float_as_int(q2.y),
                                             __float_as_int(q2.z), c.ty * kTile, c.tx * kTile, g.W, g.row_end);
            if (COUNT) {
                n_rows_hit += rows_hit;
                const int entry_rows = rows_hit + __shfl_xor(rows_hit, 1) + __shfl_xor(rows_hit, 2); // the entry's 4 threads
                n_staged_hit += (sub == 0 && entry_rows > 0) ? 1 : 0;
            }
            if (sub == 0) {
                s.rec[se][0] = q0;
                s.rec[se][1] = make_float4(q0.w, q1.x, q1.y, q1.z);
                s.rec[se][2] = make_float4(q1.w, q2.x, 0.0f, 0.0f);
                if (!COUNT) s.idx[pb][se] = idx;
            }
        }
        __syncthreads();
        if constexpr (COUNT) { // every staged entry, at its list position (32 B per staged pair)
            if (se < cnt) wave_masks[(size_t)(base + se) * 4 + sub] = s_mask[sub * B + se];
            n_staged += (tid == 0) ? (unsigned long long)cnt : 0ull;
        }
        unsigned long long touched = 0ull; // bit e: the body of entry e ran in this wave
        if (alive_mask != 0ull || COUNT) {
            const unsigned long long my_mask = (lane < cnt) ? s_mask[w * B + lane] : 0ull;
            // entries that touch a pixel of this wave's block that is still alive now (the counting build walks
            // every entry that touches the block at all, for its "visited" statistic); pixels only ever die, so
            // nothing is missed, and the per-entry test below still sees the mask of the moment
            unsigned long long cand = __ballot(COUNT ? my_mask != 0ull : (my_mask & alive_mask) != 0ull);
            while (cand != 0ull) {
                const int e = __builtin_ctzll(cand);
                cand &= cand - 1ull;
                const unsigned long long wm = readlane_u64(my_mask, e);
                if (COUNT) n_vis += (wm >> lane) & 1ull;
                const unsigned long long act = wm & alive_mask; // visited (main.cpp:511-514) and not cut off (:520)
                if (act == 0ull) continue;
                if (COUNT) n_exec += (lane == 0);
                else touched |= 1ull << e;
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
                if (COUNT) n_act += (act >> lane) & 1ull;
            }
        }
        if constexpr (COUNT) {
            if (!block_any_alive(&s.alive, w, lane, alive_mask)) break; // every pixel of the tile saturated: retire it
        } else {
            unsigned long long exec_mask;
            const bool any = block_any_alive_exec(&s.alive, s.touched, w, lane, alive_mask, touched, &exec_mask);
            // the entries some wave executed, compacted behind those of the batches before (nothing for the others)
            if ((exec_mask >> se) & 1ull) { // (se >= cnt: never executed)
                const uint32_t at = beg + n_out + (uint32_t)__popcll(exec_mask & ((1ull << se) - 1ull));
                wave_masks[(size_t)at * 4 + sub] = s_mask[sub * B + se];
                if (sub == 0) exec_list[at] = s.idx[pb][se];
            }
            n_out += (uint32_t)__popcll(exec_mask);
            if (HINT && exec_mask != 0ull) last_exec = (base - beg) + 64u - (uint32_t)__builtin_clzll(exec_mask);
            if (!any) { // every pixel of the tile saturated: retire it
                retired = true;
                break;
            }
        }
    }
    if (CHUNK) *T_io = T;
    if constexpr (THROUGHPUT) *T_io = T;
    if constexpr (COVERAGE) *ca_out = ca;
    if constexpr (HINT)
        if (tid == 0) retire_hint[c.tile] = retired ? last_exec : kNoHint;
    if (COUNT) {
        count_add(&counters->fwd_visited, n_vis, lane);
        count_add(&counters->fwd_active, n_act, lane);
        if (tid == 0) atomicAdd(&counters->fwd_staged, n_staged);
        if (lane == 0) atomicAdd(&counters->fwd_wave_execs, n_exec);
        count_add(&counters->fwd_rows_hit, n_rows_hit, lane);
        count_add(&counters->fwd_staged_hit, n_staged_hit, lane);
    }
    return n_out;
}

// Optimistic launch: the host queues the first raster kernel of an iteration before it has seen the containment flag
// the previous Adam (or projection) kernel produced.  If some splat left its binned rectangle the lists are stale:
// do nothing; the host rebuilds them and launches again.  The flag is final before the kernel starts (stream order).
// abort_stamp 0: lists known to be current.  A parameter that went non-finite in an EARLIER iteration stops the
// run where the reference abort()s (main.cpp:752-785): every later kernel of the queue does nothing.
__device__ __forceinline__ bool launch_is_void(const DeviceStatus* status, int abort_stamp, int iteration)
{
    return (abort_stamp != 0 && status->rebin_needed == abort_stamp) || status->first_nonfinite_iter < iteration;
}

static inline unsigned raster_grid(int num_tiles) { return (unsigned)(((num_tiles + 7) / 8) * 8); }

// Run-time flags -> template arguments: calls f(std::bool_constant<flag>{}...) for the values of (exact, count, half,
// further flags...); a flag given as a std::bool_constant is not branched on.  Which variants exist is decided here and
// nowhere else: exact exp is a validation mode on plain fp32 images without pair counting (s2d_create rejects the
// combinations), so those kernels are never instantiated.
template <bool EXACT, bool COUNT, bool HALF, bool... MORE, typename F>
static hipError_t with_variant(F&& f)
{
    if constexpr (EXACT && (COUNT || HALF)) return hipErrorInvalidValue;
    else return f(std::bool_constant<EXACT>{}, std::bool_constant<COUNT>{}, std::bool_constant<HALF>{},
                  std::bool_constant<MORE>{}...), hipSuccess;
}
template <bool... DONE, typename F, typename... REST>
static hipError_t with_variant(F&& f, bool flag, REST... rest)
{
    return flag ? with_variant<DONE..., true>(f, rest...) : with_variant<DONE..., false>(f, rest...);
}
template <bool... DONE, typename F, bool FLAG, typename... REST>
static hipError_t with_variant(F&& f, std::bool_constant<FLAG>, REST... rest)
{
    return with_variant<DONE..., FLAG>(f, rest...);
}

// launch_raster (s2d_raster.hip) hands a pass to the unit that holds its kernels; every backward walk ends with
// launch_det_gather, which returns the status of the launches before it.
hipError_t launch_raster_ranges(RasterPass pass, const RasterArgs& a, hipStream_t stream); // s2d_raster_ranges.hip
hipError_t launch_raster_gradient(const RasterArgs& a, hipStream_t stream);                // s2d_raster_gradient.hip
hipError_t launch_det_gather(const RasterArgs& a, hipStream_t stream);                     // s2d_raster_det.hip
hipError_t launch_raster_coverage(RasterPass pass, const RasterArgs& a, hipStream_t stream); // s2d_raster_coverage.hip

} // namespace s2d
