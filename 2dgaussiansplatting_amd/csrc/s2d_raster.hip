// s2d_raster.hip -- tile-binned forward rasteriser and analytic backward pass.
//
// One 256-thread workgroup (4 wave64) per 16x16 image tile, one thread per pixel.  Each wave owns an 8x8 pixel
// block of the tile, lane = 8 * (row in block) + (column in block).  A tile walks its splat list (ascending splat index ==
// the reference's blend order, main.cpp:419/:552) twice -- forward_tile, then backward_tile -- in batches of 64 entries
// staged in LDS:
//   * forward walk: 4 threads per entry load the 64-byte projected record and evaluate the reference's exact per-row
//     column range (solve_quadratic + int truncation, main.cpp:498-509) for 4 tile rows each, producing one
//     64-bit lane mask per (entry, wave): bit l set <=> the reference's loops visit that pixel for that
//     splat.  The quadratic is solved once per (entry, row), not per pixel.  At the end of a batch the masks and
//     splat indices of the entries whose body ran in at least one wave are stored, compacted to the front of the
//     tile's own range (32 + 4 B per executed pair); the backward walk goes through those entries only, in batches
//     of its own, and loads the masks instead of solving the quadratics again.
//   * after the barrier lane l of every wave fetches the mask of entry l; a ballot of "mask touches a live pixel" is
//     the set of entries this wave has to look at, and the blend loop iterates over its set bits only
//     (scalar bit tricks + v_readlane), skipping an entry with a scalar branch when no lane is live any more.
// A pixel whose throughput fell below 1/256 never works again (main.cpp:520); when all 256 pixels of the tile
// are in that state the workgroup stops walking its list (tile retirement).
//
// Kernels: raster_fused_kernel runs both walks of a tile in one launch, the final colours staying in registers
// (what s2d_step and s2d_forward_backward queue); raster_forward_kernel / raster_backward_kernel run one walk each
// through image0 (s2d_forward / s2d_backward, and the counting diagnostics).
//
// The alpha / throughput / colour arithmetic is the reference's, operation for operation
// (-ffp-contract=off), in both walks, so the framebuffer is bit-identical to the oracle's and the backward
// walk makes exactly the forward's per-pixel decisions.  The backward walk then sums each splat's nine
// partial gradients over the wave through an LDS transpose (wave_sum8_lds), over the four waves in one LDS slot per
// entry, and issues one global float-atomic burst per (tile, splat) into the N x 9 gradient array -- or,
// with S2D_CFG_DETERMINISTIC, keeps one slot per wave, adds them in a fixed order and stores the partial into the
// tile's own slot of that splat, and a gather kernel sums each splat's slots in a fixed order (bitwise
// reproducible gradients).
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

// What the backward walk starts from, per pixel: the reference's own dL/dC = finalColor - imageRef (main.cpp:616), or --
// UPSTREAM -- the caller's dL/d(image0) of some other loss.  The backward kernels' image_ref is then that gradient image:
// RGBA32F whatever the image format, one 16-byte load per pixel, .w not used, 0 for lanes outside the image.
template <bool HALF, bool UPSTREAM>
__device__ __forceinline__ float4 load_ref_or_upstream(const void* src, size_t i)
{
    return UPSTREAM ? reinterpret_cast<const float4*>(src)[i] : load_pixel<HALF>(src, i);
}
// (By value on purpose: handed over as whole 16-byte values, the way backward_tile took `ref` before, the kernels without
// UPSTREAM compile to the instructions they had when the subtraction stood inside backward_tile -- DESIGN.md section 10;
// by reference the compiler narrows their image loads and renumbers registers.)
template <bool UPSTREAM>
__device__ __forceinline__ float4 loss_grad(const float4 fin, const float4 src)
{
    return UPSTREAM ? src : make_float4(fin.x - src.x, fin.y - src.y, fin.z - src.z, 0.0f);
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
template <bool COUNT, bool EXACT, bool CHUNK = false>
__device__ __forceinline__ uint32_t forward_tile(FwdShared& s, const TileCtx& c, const uint32_t* __restrict__ tile_off,
                                             const uint32_t* __restrict__ list, const ProjRec* __restrict__ proj,
                                             unsigned long long* __restrict__ wave_masks, uint32_t* __restrict__ exec_list,
                                             uint32_t* __restrict__ retire_hint, const Geometry& g,
                                             PairCounters* __restrict__ counters, f2& crg, float& cb, float* T_io = nullptr)
{
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
                // Branch-free body: lanes outside `act` run the same instructions with alpha forced to 0, which
                // makes c += (T*c)*0 and T *= 1 exact no-ops.  The scalar mask itself is the select predicate.
                const float4 q0 = s.rec[e][0], q1 = s.rec[e][1], q2 = s.rec[e][2];
                const f2 v = pxy - mk2(q0.x, q0.y);                          // main.cpp:523-524
                const f2 m = mk2(q0.z, q0.w) * v.x + mk2(q1.x, q1.y) * v.y;  // inv_cov * v: (a vx + b vy, b vx + d vy)
                const f2 vm = v * m;
                bool nonzero;
                const float G = gauss_of<EXACT>(vm.x + vm.y, &nonzero);         // main.cpp:526-527
                const unsigned long long on = act & __ballot(nonzero);
                const float alpha = __builtin_amdgcn_inverse_ballot_w64(on) ? G * q2.y : 0.0f;
                crg += (T * mk2(q1.z, q1.w)) * alpha;                        // main.cpp:529-530: (T*c)*alpha
                cb += T * q2.x * alpha;                                      // main.cpp:531
                T *= (1.0f - alpha);                                         // main.cpp:533
                alive_mask &= __ballot(!(T < kMinThroughput));               // main.cpp:520, for the next splat
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

template <bool COUNT, bool HALF, bool EXACT>
__global__ __launch_bounds__(256) void raster_forward_kernel(const uint32_t* __restrict__ tile_off,
                                                             const uint32_t* __restrict__ list,
                                                             const ProjRec* __restrict__ proj,
                                                             void* __restrict__ image0,
                                                             unsigned long long* __restrict__ wave_masks,
                                                             uint32_t* __restrict__ exec_list, uint32_t* __restrict__ tile_exec,
                                                             uint32_t* __restrict__ retire_hint,
                                                             Geometry g, const DeviceStatus* __restrict__ status, int abort_stamp,
                                                             int iteration, PairCounters* __restrict__ counters)
{
    __shared__ FwdShared s;
    if (launch_is_void(status, abort_stamp, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    f2 crg;
    float cb;
    const uint32_t n_exec = forward_tile<COUNT, EXACT>(s, c, tile_off, list, proj, wave_masks, exec_list, retire_hint, g, counters, crg, cb);
    if (!COUNT && c.tid == 0) tile_exec[tile] = n_exec; // the backward walk is another launch
    if (c.inside) store_pixel<HALF>(image0, pixel_index(c, g), make_float4(crg.x, crg.y, cb, 1.0f)); // .w reset, main.cpp:543-546
}

// ---------------------------------------------------------------------------------------------------
// Wave-wide sums of eight of the nine partial gradients, through LDS.
// On gfx950 a v_permlane*_swap occupies the SIMD for ~8.8 cycles and a DPP add for ~4.6 against 2.4 for a plain
// v_add_f32 (tools/microbench/valu_rates.hip), so a swap/DPP butterfly costs ~90 SIMD cycles per (wave, entry) of a
// VALU-bound kernel (profiles/r01/v9_bench_lds_reduce.json), while the LDS pipe idles.  Here every lane stores its 8 partials component-major into a
// wave-private scratch (element n = 64*c + lane), reads back elements 8*lane .. 8*lane+7 -- eight lanes' worth of
// component lane>>3 -- with two 16-B reads, adds them pairwise (7 plain adds) and finishes inside its 8-lane
// group with three DPP adds: ~31 SIMD cycles.  Afterwards every lane of group g = lane >> 3 holds the total of
// component g.  Element n lives at dword n + 4*(n >> 7): a ds_read_b128 is served in four groups of sixteen lanes --
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 (MI355X_MICROARCH.md, LDS) -- over 64 banks, and with
// 32-byte strides the sixteen lanes of a group would cover the banks twice; shifting the runs of lanes 16-31 (32-47,
// 48-63) by one (two, three) 16-byte pads puts the lanes of every group on sixteen different quads of banks.  (Rounds 1-3
// padded every 32 elements, which is 2-way conflicted under this grouping, as is a pad every 64: SQ_LDS_BANK_CONFLICT
// 85 M -> 15 M cycles per launch, +0.7...1.3 %, profiles/r03/ab_lds_and_salu.txt.)  The stores are 32 consecutive dwords
// per half-wave either way.  Same-wave LDS accesses complete in issue order, so no barrier is needed -- only the compiler
// is told not to reorder.
// The ninth value (opacity gradient) takes the DPP chain to lane 63, interleaved with the group sum.
// ---------------------------------------------------------------------------------------------------
constexpr int kPadShift = 7; // element n lives at dword n + 4 * (n >> kPadShift)
static_assert(kPadShift >= 6, "a pad inside a component's 64 elements would make the store address lane-dependent");
constexpr int red_at(int n) { return n + 4 * (n >> kPadShift); }
constexpr int kRedDwords = red_at(512); // per wave

template <bool NINTH>
__device__ __forceinline__ float wave_sum8_lds(float* sw, int lane, float a0, float a1, float a2, float a3, float a4,
                                               float a5, float a6, float a7, float& a8)
{
    float* wp = sw + lane; // (a component's 64 elements never straddle a pad)
    wp[red_at(0 * 64)] = a0;
    wp[red_at(1 * 64)] = a1;
    wp[red_at(2 * 64)] = a2;
    wp[red_at(3 * 64)] = a3;
    wp[red_at(4 * 64)] = a4;
    wp[red_at(5 * 64)] = a5;
    wp[red_at(6 * 64)] = a6;
    wp[red_at(7 * 64)] = a7;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float4* rp = reinterpret_cast<const float4*>(sw + 8 * lane + 4 * (lane >> (kPadShift - 3)));
    const float4 u = rp[0], v = rp[1];
    float t = ((u.x + u.y) + (u.z + u.w)) + ((v.x + v.y) + (v.z + v.w));
    // the reads must have returned before the next entry's stores may be issued by the compiler
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (NINTH) {
        asm volatile("s_nop 1\n"
                     "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                     "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                     "s_nop 0\n"
                     "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
                     "v_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
                     "s_nop 0\n"
                     "v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n"
                     "v_add_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n"
                     "s_nop 1\n"
                     "v_add_f32_dpp %1, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n"
                     "s_nop 1\n"
                     "v_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n"
                     "s_nop 1\n"
                     "v_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n"
                     "s_nop 1\n"
                     : "+v"(t), "+v"(a8));
    } else {
        asm volatile("s_nop 1\n"
                     "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                     "s_nop 1\n"
                     "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
                     "s_nop 1\n"
                     "v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n"
                     "s_nop 1\n"
                     : "+v"(t));
    }
    return t;
}

// num / den as IEEE division would round it, from the hardware reciprocal r = v_rcp_f32(den) (1 ulp) shared by several
// numerators: quotient estimate, then ONE correction q += (num - den*q) * r whose residual is exact (fma).  The estimate
// is off by up to ~1.5 ulp.  Measured on 3 x 10^8 operand pairs of this blend's range, den = 1e-15 and quotients next to
// rounding midpoints included (tools/check_recip_division.py, profiles/r04/r04_recip_division_check.txt): with a correctly
// rounded r the corrected value is the IEEE quotient in every trial; with r one ulp off, 7-9 quotients per 10^8 differ from
// IEEE division (1-2 per 10^8 after a second correction) -- at ~10^9 quotients per iteration of 4096^2 / 1 M that is at most a
// few dozen one ulp off per iteration.  Rounds 1-3 applied two corrections: six more instructions per executed (wave, entry),
// same parity statistics, -2.9 % (profiles/r03/ab_one_division_correction.txt).  No per-division scaling for denormal / huge
// operands: they cannot occur here (den in {1e-15} u [2^-24, 1], |num| <~ 1).
// The quotient should be the one the reference computes:
// c*T - S/(1-alpha) cancels down to a T_final-sized remainder, which magnifies a last-place difference in the
// quotient by T/T_final (10^3..10^5 in flat image regions); the gradient bars are what is asserted.
__device__ __forceinline__ float div_by_recip(float num, float den, float r)
{
    const float q = num * r;
    return __builtin_fmaf(__builtin_fmaf(-den, q, num), r, q);
}

// ---------------------------------------------------------------------------------------------------
// backward, main.cpp:548-712, + the squared error of main.cpp:796-805
//
// Per (pixel, splat) the reference adds nine terms (main.cpp:619, :654-655, :677-678, :685, :704).  They are
// evaluated with the reference's own expressions: its three-term dot products (cc vx^2 + 2sc vx vy + ss vy^2,
// ...) and the channel sum dL . dC/dalpha can cancel, and then carry rounding noise that only the same
// operation order reproduces (the algebraically equal alpha*u^2/sx^3 with u = cos*vx + sin*vy is cheaper and
// more accurate, but differs from the reference by up to 1e-4 of a splat's summed |terms| when its few live
// pixels lie near u = 0).  Only factors that are plain products are regrouped or precomputed per entry
// (1/sx^3, 1/sy^3, (sx^2-sy^2)/(sx^2 sy^2), 0.5*alpha*(2a vx + (b+c) vy) = alpha*mx): a few ulp per term.
// ---------------------------------------------------------------------------------------------------
// Where a tile puts its partial gradient of a splat in deterministic mode.
struct DetSlots {
    const TileRect* rects;     // per splat: the rectangle its pairs were emitted from
    const uint32_t* offsets;   // per splat: first emission slot
    float* data;               // [pairs][kDetStride]: nine floats per slot, padded to three 16-byte words
    uint32_t* stamp;           // [pairs]: iteration + 1 of the last write
    uint32_t* touched;         // [splats]: bit j = slot offsets[i] + j was written in this pass (bit 31: some slot >= 31)
    uint32_t now;              // iteration + 1
};

// LDS of the backward walk.  Entries per staged batch: 64, or 32 in deterministic mode, whose four per-wave slot sets would
// otherwise lift the workgroup from 18.9 to ~25 KB of LDS -- six instead of eight workgroups per CU, which alone costs
// ~14 % (profiles/r03/r03_bound_experiments.txt); with half-size batches it is 17.1 KB.
// STATS (the density-statistics walk): a slot also carries |dpos.x|, |dpos.y| and the blend weight in
// words 9..11, so deterministic mode's per-wave slots are 12 floats too (18.6 KB); nothing else changes.
template <bool DET, bool STATS = false>
struct BwdShared {
    static constexpr int kBatch = DET ? 32 : B;
    float4 q0[kBatch]; // pos.x, pos.y, a, b
    float4 q1[kBatch]; // b, d, col_r, col_g
    float4 q2[kBatch]; // col_b, opacity, (sx^2-sy^2)/(sx^2 sy^2), sin*cos
    float4 e0[kBatch]; // cc, ss, 2sc, cc - ss
    float4 e1[kBatch]; // ss, cc, 1/sx^3, 1/sy^3
    unsigned long long mask[4 * kBatch]; // [wave][entry]
    // Partial gradients of the batch, 9 floats per slot (+3 pad where one slot per entry is shared).  Deterministic mode:
    // one slot per wave, plain stores, summed over the 4 waves in a fixed order by the flush.  Otherwise the four waves add into ONE slot
    // per entry with ds_add_f32 (eight lanes, eight addresses per wave and entry): the order of those four
    // additions is as free as the order of the global atomics that follow, and 9 KB less LDS per workgroup is
    // one to two more resident workgroups per CU.  The flush zeroes what it read.
    static constexpr int kPartStride = (DET && !STATS) ? 9 : 12; // floats per slot (deterministic mode packs its four slots per entry tightly)
    __attribute__((aligned(16))) float part[(DET ? 4 : 1) * kBatch * kPartStride];
    // Splat index of each staged entry: the flush addresses gradients without going back to the list.  Two copies, by batch
    // parity: a batch's flush runs behind the last barrier of the batch, so fast threads already stage the NEXT batch
    // (and overwrite these words) while slow ones still flush.  Deterministic mode also keeps the entry's slot for this
    // tile and which of the splat's slots that is.
    uint32_t idx[2][kBatch];
    uint32_t slot[2][DET ? kBatch : 1];
    uint32_t local[2][DET ? kBatch : 1];
    unsigned long long touched[4]; // bit e: wave w wrote slot e in this batch
    double red[4];
    int4 alive;                    // per wave: does it still have a live pixel (block_any_alive)
    int last_tile;                 // this workgroup stored the launch's last tile error: it adds them all up
    __attribute__((aligned(16))) float xpose[4][kRedDwords]; // wave-private transpose scratch
};

// One tile's backward walk (main.cpp:552-711 for its pixels) from the pixel's final colour `fin` and the loss gradient
// `dL` = dL/dC of that pixel (.w unused; the reference's own loss: fin - ref, main.cpp:616, formed by the caller):
// adds the tile's partial gradients into grads (or its deterministic slots) and stores the tile's squared error.
// UPSTREAM: dL is a caller's gradient of some other loss, so there is no squared error to form -- no reduction, no
// tile_sqerr store, no ticket (tile_sqerr and sq are not looked at).
// It walks the n_handed entries the forward walk handed over (exec_list, wave_masks: see forward_tile), every one of which
// has a body to run in some wave; a counting walk (COUNT) goes through the tile's whole list and ignores both.
// CHUNK: as in forward_tile -- the list is one index range of the splats, *state_io (running colour r, g, b and T of
// main.cpp:601-625, :707) is the pixel's state after the ranges before it on entry and after this range on return.
// STATS: next to the nine gradients the walk sums |g_px|, |g_py| and alpha * T (the blend weight, main.cpp:618) of every
// (pixel, splat) the reference's body reaches -- words 9..11 of the same slots, flushed into `stats` (n x 3 floats, float
// atomics) or, in deterministic mode, into words 9..11 of the tile's global slot for gather_stats_kernel.
template <bool COUNT, bool NEED_OP, bool DET, bool EXACT, bool CHUNK = false, bool UPSTREAM = false, bool STATS = false>
__device__ __forceinline__ void backward_tile(BwdShared<DET, STATS>& s, const TileCtx& c, const float4 fin, const float4 dL,
                                              const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ list,
                                              const ProjRec* __restrict__ proj,
                                              const unsigned long long* __restrict__ wave_masks,
                                              const uint32_t* __restrict__ exec_list, uint32_t n_handed,
                                              float* __restrict__ grads, double* __restrict__ tile_sqerr,
                                              const Geometry& g, const DetSlots& det, PairCounters* __restrict__ counters,
                                              const SqerrJob& sq, float4* state_io = nullptr, float* __restrict__ stats = nullptr)
{
    using Shared = BwdShared<DET, STATS>;
    constexpr int BB = Shared::kBatch;      // entries per staged batch
    constexpr int KF = STATS ? 12 : 9;      // floats of a slot the flush moves
    const int tid = c.tid, lane = c.lane, w = c.w;
    const bool inside = c.inside;
    const f2 pxy = c.pxy;
    // after wave_sum8_lds the 8-lane group holds the total of component lane >> 3, and lane 63 the ninth sum (slot 8)
    const bool op_lane = NEED_OP && !DET && lane == 63;
    const int part_slot = op_lane ? 8 : lane >> 3;
    const bool adds = (lane & 7) == 0 || op_lane;
    const float dLr = dL.x, dLg = dL.y, dLb = dL.z; // dL_dC, main.cpp:616
    const f2 dLrg = mk2(dLr, dLg), fin_rg = mk2(fin.x, fin.y);

    // squared error of this tile (main.cpp:801-802): float per pixel, double across pixels
    if constexpr (!UPSTREAM) {
        const float ex = dLr * 255.0f, ey = dLg * 255.0f, ez = dLb * 255.0f;
        double e2 = inside ? (double)(ex * ex + ey * ey + ez * ez) : 0.0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) e2 += __shfl_down(e2, d, 64);
        if (lane == 0) s.red[w] = e2;
    }
    if (!DET)
        for (int i = tid; i < BB * 3; i += 256) reinterpret_cast<float4*>(s.part)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    if constexpr (UPSTREAM) {
        // (no squared error: the loss is the caller's)
    } else if (sq.out == nullptr) {
        if (tid == 0) tile_sqerr[c.tile] = ((s.red[0] + s.red[1]) + s.red[2]) + s.red[3];
    } else {
        // Small images: the iteration's squared error (main.cpp:796-805) is summed here, by the workgroup whose tile
        // error completes the set (a ticket behind the stores), instead of by a launch of its own.
        if (tid == 0) {
            __hip_atomic_store(tile_sqerr + c.tile, ((s.red[0] + s.red[1]) + s.red[2]) + s.red[3], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
            unsigned long long* ticket = reinterpret_cast<unsigned long long*>(sq.scratch + kSqerrChunks);
            s.last_tile = atomicAdd(ticket, 1ull) == (unsigned long long)(sq.num_tiles - 1) ? 1 : 0;
        }
        __syncthreads();
        if (s.last_tile) { // block-uniform
            __threadfence();
            const double total = sqerr_sum_small(tile_sqerr, sq.num_tiles, s.red);
            if (tid == 0) {
                *sq.out = total;
                *reinterpret_cast<unsigned long long*>(sq.scratch + kSqerrChunks) = 0ull;
            }
        }
    }

    f2 crg = mk2(0.0f, 0.0f);                        // image1 = (0,0,0,1), main.cpp:549
    float cb = 0.0f, T = 1.0f;
    if (CHUNK) {
        crg = mk2(state_io->x, state_io->y);
        cb = state_io->z;
        T = state_io->w;
    }
    unsigned long long alive_mask = __ballot(CHUNK ? inside && !(T < kMinThroughput) : inside); // wave-uniform, scalar registers (see the forward kernel)
    unsigned long long n_vis = 0, n_act = 0, n_staged = 0, n_exec = 0;

    const uint32_t beg = tile_off[c.tile];
    const uint32_t end = beg + (COUNT ? tile_off[c.tile + 1] - beg : n_handed);
    const int se = tid >> 2, sub = tid & 3;
    for (uint32_t base = beg; base < end; base += BB) {
        const int cnt = (int)min((uint32_t)BB, end - base);
        const int pb = (int)(((base - beg) / (uint32_t)BB) & 1u); // which copy of the per-entry index words this batch uses
        if (se < cnt) {
            // the forward pass of this iteration left the lane masks behind
            s.mask[sub * BB + se] = wave_masks[(size_t)(base + se) * 4 + sub];
            if (sub == 0) {
                const uint32_t idx = COUNT ? list[base + se] : exec_list[base + se];
                s.idx[pb][se] = idx;
                if (DET) { // the slot of this tile in the splat's emission rectangle (row-major), looked up beside the record
                    const TileRect r = det.rects[idx];
                    const uint32_t local = (uint32_t)(c.ty - g.trow0 - r.ty0) * (uint32_t)(r.tx1 - r.tx0 + 1) + (uint32_t)(c.tx - r.tx0);
                    s.slot[pb][se] = det.offsets[idx] + local;
                    s.local[pb][se] = min(local, 31u);
                }
                const ProjRec* r = proj + idx;
                const float4 q0 = r->q0, q1 = r->q1, q2 = r->q2;
                const float4 q3 = r->q3; // sin, 1/sx^3, 1/sy^3, (sx^2-sy^2)/(sx^2 sy^2): divided once per splat (pack_proj)
                const float cosT = q2.w, sinT = q3.x;
                const float cc = cosT * cosT, ss = sinT * sinT, sc2 = 2.0f * sinT * cosT;
                s.q0[se] = q0;
                s.q1[se] = make_float4(q0.w, q1.x, q1.y, q1.z);
                s.q2[se] = make_float4(q1.w, q2.x, q3.w, sinT * cosT);
                s.e0[se] = make_float4(cc, ss, sc2, cc - ss);
                s.e1[se] = make_float4(ss, cc, q3.y, q3.z);
            }
        }
        __syncthreads();
        if (COUNT) n_staged += (tid == 0) ? (unsigned long long)cnt : 0ull;
        unsigned long long touched = 0ull;
        if (alive_mask != 0ull || COUNT) {
            const unsigned long long my_mask = (lane < cnt) ? s.mask[w * BB + lane] : 0ull;
            unsigned long long cand = __ballot(COUNT ? my_mask != 0ull : (my_mask & alive_mask) != 0ull); // as in the forward walk
            while (cand != 0ull) {
                const int e = __builtin_ctzll(cand);
                cand &= cand - 1ull;
                const unsigned long long wm = readlane_u64(my_mask, e);
                if (COUNT) n_vis += (wm >> lane) & 1ull;
                const unsigned long long act_mask = wm & alive_mask;
                if (act_mask == 0ull) continue;
                touched |= 1ull << e;
                if (COUNT) n_exec += (lane == 0);
                // Lanes this splat does not visit (main.cpp:595-598) or whose pixel is already below the throughput
                // cut-off (main.cpp:604) run the same instructions with alpha forced to 0: then c += T*c*0 and
                // T *= 1 are exact no-ops and every gradient term below is a multiple of alpha, i.e. exactly 0 --
                // no divergent region, no zero-initialisation of the nine partials.
                if (COUNT) {
                    n_act += (act_mask >> lane) & 1ull;
                    const int na = __popcll(act_mask);
                    if (lane == 0) atomicAdd(&counters->bwd_lane_hist[na], 1ull);
                    // how many of the block's four 4x4 quadrants have a live covered pixel (lane = 8*row + column)
                    const uint32_t lo = (uint32_t)act_mask, hi = (uint32_t)(act_mask >> 32);
                    const int nq = ((lo & 0x0F0F0F0Fu) != 0u) + ((lo & 0xF0F0F0F0u) != 0u) + ((hi & 0x0F0F0F0Fu) != 0u) +
                                   ((hi & 0xF0F0F0F0u) != 0u);
                    if (lane == 0) atomicAdd(&counters->bwd_quadrant_execs, (unsigned long long)nq);
                }
                float g_px, g_py, g_sx, g_sy, g_rot, g_r, g_g, g_b, g_op = 0.f;
                float st_w = 0.f; // STATS: alpha * T of this pixel
                {
                    const float4 q0 = s.q0[e], q1 = s.q1[e], q2 = s.q2[e];
                    const float4 e0 = s.e0[e], e1 = s.e1[e];
                    // ---- the reference's operations, in its order (decides T, alive, the running colour) ----
                    const f2 v = pxy - mk2(q0.x, q0.y);                              // main.cpp:607-608
                    const f2 m = mk2(q0.z, q0.w) * v.x + mk2(q1.x, q1.y) * v.y;      // inv_cov * v
                    const f2 vm = v * m;
                    bool nonzero;
                    const float G = gauss_of<EXACT>(vm.x + vm.y, &nonzero);          // main.cpp:609-610
                    // one scalar mask selects alpha (and dOpacity): visited, alive, and G not cut to 0
                    const bool on = __builtin_amdgcn_inverse_ballot_w64(act_mask & __ballot(nonzero));
                    const float alpha = on ? G * q2.y : 0.0f;                        // main.cpp:611
                    const f2 Trg = T * mk2(q1.z, q1.w);
                    const float Tb = T * q2.x;
                    crg += Trg * alpha;                                              // main.cpp:623-625
                    cb += Tb * alpha;
                    // ---- gradient terms ----
                    const float dC_dc = alpha * T;                                   // main.cpp:618
                    const f2 g_rg = dLrg * dC_dc;
                    g_r = g_rg.x;
                    g_g = g_rg.y;
                    g_b = dLb * dC_dc;
                    if constexpr (STATS) st_w = dC_dc;
                    // S / (1 - alpha + 1e-15), main.cpp:627-628: three quotients over one denominator (div_by_recip)
                    const float den = 1.0f - alpha + 1.0e-15f;
                    const float rd = __builtin_amdgcn_rcpf(den); // 1 ulp; the correction below does the rest
                    const f2 S_rg = fin_rg - crg;                                    // S = final - colour
                    const f2 nden2 = mk2(-den, -den), rd2 = mk2(rd, rd);
                    f2 q_rg = S_rg * rd;
                    q_rg = fma2(fma2(nden2, q_rg, S_rg), rd2, q_rg);
                    const f2 dCa_rg = Trg - q_rg;
                    const float dCa_b = Tb - div_by_recip(fin.z - cb, den, rd);
                    // the three channel products may cancel: same products, same order as main.cpp:629-630
                    const f2 pr = dLrg * dCa_rg;
                    const float gs = (pr.x + pr.y) + dLb * dCa_b;
                    const float ga = gs * alpha;
                    const f2 g_pos = ga * m;                                         // main.cpp:639-640, :654-655
                    g_px = g_pos.x;
                    g_py = g_pos.y;
                    const f2 vv = v.x * v;                                           // vx*vx, vx*vy
                    const float vyy = v.y * v.y;
                    // both covariance dot products (main.cpp:657-662): (cc, ss)*vxx +- 2sc*vxy, then + (ss, cc)*vyy
                    // (x + (-2sc)*vxy and x - 2sc*vxy are the same IEEE operation)
                    const float sc2vxy = e0.z * vv.y;
                    const f2 dots = mk2(e0.x * vv.x + sc2vxy, e0.y * vv.x - sc2vxy) + mk2(e1.x, e1.y) * vyy;
                    const f2 g_s = (ga * mk2(e1.z, e1.w)) * dots;                    // main.cpp:657-662, :677-678
                    g_sx = g_s.x;
                    g_sy = g_s.y;
                    g_rot = (ga * q2.z) * (e0.w * v.x * v.y - q2.w * (vv.x - vyy)); // main.cpp:680-685, e0.w = cc - ss
                    if (NEED_OP) g_op = on ? gs * G : 0.0f;                           // main.cpp:703-704
                    T *= (1.0f - alpha);                                             // main.cpp:707
                    alive_mask &= __ballot(!(T < kMinThroughput));
                }
                // order of the record: pos.xy, sx, sy, rot, color.rgb, opacity (main.cpp:85-93)
                const float tot = wave_sum8_lds<NEED_OP>(s.xpose[w], lane, g_px, g_py, g_sx, g_sy, g_rot, g_r, g_g, g_b, g_op);
                // slot of (wave, entry, component), 12 dwords per entry.  The entry's share of the index is computed on the
                // scalar unit explicitly: left to itself the compiler folds e * 12 + lane term into a per-lane
                // v_mad_u64_u32 in the blend loop.
                float* const part = s.part;
                int pe;
                asm("s_mul_i32 %0, %1, %2" : "=s"(pe) : "s"((DET ? __builtin_amdgcn_readfirstlane(w) : 0) * BB + e), "n"(Shared::kPartStride));
                if (DET) {
                    if ((lane & 7) == 0) part[pe + part_slot] = tot;
                    if (NEED_OP && lane == 63) part[pe + 8] = g_op;
                } else {
                    const float val = op_lane ? g_op : tot; // one LDS instruction for the eight totals and the ninth sum
                    if (adds) __hip_atomic_fetch_add(part + (pe + part_slot), val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if constexpr (STATS) {
                    // a second round of the same transpose: the totals of |g_px|, |g_py| and alpha * T end in the 8-lane
                    // groups 0..2 (lanes outside the reference's body hold exact zeros: every term is a multiple of alpha)
                    float none = 0.f;
                    const float st = wave_sum8_lds<false>(s.xpose[w], lane, __builtin_fabsf(g_px), __builtin_fabsf(g_py), st_w, 0.f, 0.f,
                                                          0.f, 0.f, 0.f, none);
                    if ((lane & 7) == 0 && lane < 24) {
                        if (DET) part[pe + 9 + (lane >> 3)] = st;
                        else __hip_atomic_fetch_add(part + (pe + 9 + (lane >> 3)), st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
        if (DET && lane == 0) s.touched[w] = touched;
        // (the handed-over entries end with the last one any pixel was alive for: only a counting walk can retire early)
        bool any = true;
        if constexpr (COUNT) any = block_any_alive(&s.alive, w, lane, alive_mask);
        else __syncthreads();
        // one burst per (tile, splat): 9 consecutive floats -- float atomics into grads[idx], or (deterministic
        // mode) plain stores into this tile's own slot of the splat, summed later in a fixed order
        for (int i = tid; i < cnt * KF; i += 256) {
            const int e = i / KF, k = i - e * KF;
            if (!NEED_OP && k == 8 && !DET) continue; // dSplats.opacity left at zero on request
            float v = 0.0f;
            bool any_w = false;
            if (DET) {
#pragma unroll
                for (int ww = 0; ww < (DET ? 4 : 1); ww++)
                    if ((s.touched[ww] >> e) & 1ull) {
                        v += s.part[(ww * BB + e) * Shared::kPartStride + k];
                        any_w = true;
                    }
            } else {
                float* slot = s.part + e * Shared::kPartStride + k;
                v = *slot;
                *slot = 0.0f; // the next batch's waves add after the staging barrier
                any_w = true;
            }
            if (DET) {
                if (any_w) {
                    const uint32_t slot = s.slot[pb][e];
                    det.data[(size_t)slot * kDetStride + k] = (!NEED_OP && k == 8) ? 0.0f : v;
                    if (k == 0) {
                        det.stamp[slot] = det.now;
                        atomicOr(det.touched + s.idx[pb][e], 1u << s.local[pb][e]); // which slots the gather pass has to read
                    }
                }
            } else if (any_w && v != 0.0f) {
                if (STATS && k >= 9) atomicAdd(stats + (size_t)s.idx[pb][e] * 3 + (k - 9), v);
                else atomicAdd(grads + (size_t)s.idx[pb][e] * 9 + k, v);
            }
        }
        if (!any) break;
    }
    if (CHUNK) *state_io = make_float4(crg.x, crg.y, cb, T);
    if (COUNT) {
        count_add(&counters->bwd_visited, n_vis, lane);
        count_add(&counters->bwd_active, n_act, lane);
        if (tid == 0) atomicAdd(&counters->bwd_staged, n_staged);
        if (lane == 0) atomicAdd(&counters->bwd_wave_execs, n_exec);
    }
}

// The per-splat statistics array of a STATS kernel (n x 3 floats) is one trailing argument that only those kernels have:
// the argument list of every other instantiation, and with it the kernel as the compiler emits it, stays what it was.
__device__ __forceinline__ float* stats_of() { return nullptr; }
__device__ __forceinline__ float* stats_of(float* p) { return p; }

// UPSTREAM (both backward kernels): image_ref is not the target but the caller's dL/d(image0), see load_ref_or_upstream.
// STATS: backward_tile's density statistics (never with COUNT or EXACT).
template <bool COUNT, bool NEED_OP, bool HALF, bool DET, bool EXACT, bool UPSTREAM = false, bool STATS = false, typename... STATS_OUT>
__global__ __launch_bounds__(256) void raster_backward_kernel(const uint32_t* __restrict__ tile_off,
                                                              const uint32_t* __restrict__ list,
                                                              const ProjRec* __restrict__ proj,
                                                              const void* __restrict__ image0,
                                                              const void* __restrict__ image_ref,
                                                              const unsigned long long* __restrict__ wave_masks,
                                                              const uint32_t* __restrict__ exec_list,
                                                              const uint32_t* __restrict__ tile_exec,
                                                              float* __restrict__ grads,
                                                              double* __restrict__ tile_sqerr, Geometry g,
                                                              DetSlots det, const DeviceStatus* __restrict__ status,
                                                              int iteration, PairCounters* __restrict__ counters,
                                                              STATS_OUT... stats_out)
{
    static_assert(sizeof...(STATS_OUT) == (STATS ? 1 : 0) && !(STATS && (COUNT || EXACT)), "float* stats for the STATS kernels alone");
    __shared__ BwdShared<DET, STATS> s;
    if (launch_is_void(status, 0, iteration)) return; // the reference abort()ed in an earlier iteration
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    float4 fin = make_float4(0.f, 0.f, 0.f, 0.f), ref = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c.inside) {
        fin = load_pixel<HALF>(image0, pixel_index(c, g));    // finalColor, main.cpp:613
        ref = load_ref_or_upstream<HALF, UPSTREAM>(image_ref, pixel_index(c, g));
    }
    const uint32_t n_exec = COUNT ? 0u : tile_exec[tile];
    backward_tile<COUNT, NEED_OP, DET, EXACT, false, UPSTREAM, STATS>(s, c, fin, loss_grad<UPSTREAM>(fin, ref), tile_off, list, proj, wave_masks, exec_list, n_exec, grads, tile_sqerr,
                                              g, det, counters, SqerrJob{nullptr, 0, nullptr, nullptr}, nullptr, stats_of(stats_out...));
}

// Forward and backward walk of a tile in ONE launch (what s2d_step and s2d_forward_backward queue): a tile's backward
// pass needs nothing but its own pixels' final colours, which are still in registers when the forward walk ends.  One
// dispatch, one ramp-down tail and one read of image0 (16 B per pixel) less per iteration than the two kernels above,
// which remain for callers that run the passes separately.  The executed entries still travel through exec_list and
// wave_masks: written by the entry's staging threads and read back by other threads of the same workgroup (so they rarely
// leave L2); the __syncthreads() between the walks orders the two at workgroup scope, and their number stays in a
// register (tile_exec is written for an s2d_backward that may follow).  With S2D_CFG_FP16_IMAGES the backward walk sees the
// final colour as stored, i.e. rounded to fp16, exactly like the separate kernels.  image0 is written only when
// `write_image` is set (s2d_step: the last iteration of the call; nothing else reads it).
template <bool NEED_OP, bool HALF, bool DET, bool EXACT>
__global__ __launch_bounds__(256, 8) void raster_fused_kernel(const uint32_t* __restrict__ tile_off,
                                                           const uint32_t* __restrict__ list,
                                                           const ProjRec* __restrict__ proj, void* __restrict__ image0,
                                                           const void* __restrict__ image_ref,
                                                           unsigned long long* __restrict__ wave_masks,
                                                           uint32_t* __restrict__ exec_list, uint32_t* __restrict__ tile_exec,
                                                           uint32_t* __restrict__ retire_hint,
                                                           float* __restrict__ grads, double* __restrict__ tile_sqerr,
                                                           Geometry g, DetSlots det,
                                                           const DeviceStatus* __restrict__ status, int abort_stamp,
                                                           int iteration, int write_image, SqerrJob sq)
{
    constexpr size_t kBytes = sizeof(BwdShared<DET>) > sizeof(FwdShared) ? sizeof(BwdShared<DET>) : sizeof(FwdShared);
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes]; // the two walks use the same LDS one after the other
    if (launch_is_void(status, abort_stamp, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    f2 crg;
    float cb;
    const uint32_t n_exec = forward_tile<false, EXACT>(*reinterpret_cast<FwdShared*>(smem), c, tile_off, list, proj, wave_masks,
                                                       exec_list, retire_hint, g, nullptr, crg, cb);
    if (c.tid == 0) tile_exec[tile] = n_exec;
    float4 fin = make_float4(crg.x, crg.y, cb, 1.0f), ref = make_float4(0.f, 0.f, 0.f, 0.f);
    if (HALF) { // what the backward pass would read back from the fp16 framebuffer
        const __half2 a = __floats2half2_rn(fin.x, fin.y), b = __floats2half2_rn(fin.z, fin.w);
        const float2 fa = __half22float2(a), fb = __half22float2(b);
        fin = make_float4(fa.x, fa.y, fb.x, fb.y);
    }
    if (c.inside) {
        if (write_image) store_pixel<HALF>(image0, pixel_index(c, g), fin); // .w reset, main.cpp:543-546
        ref = load_pixel<HALF>(image_ref, pixel_index(c, g));
    } else {
        fin = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the backward walk re-uses the LDS the forward walk's hand-over may still be reading, and reads what other threads
    // of the workgroup handed over through global memory
    __syncthreads();
    backward_tile<false, NEED_OP, DET, EXACT>(*reinterpret_cast<BwdShared<DET>*>(smem), c, fin, loss_grad<false>(fin, ref), tile_off,
                                              list, proj, wave_masks, exec_list, n_exec, grads, tile_sqerr, g, det, nullptr, sq);
}

// ---------------------------------------------------------------------------------------------------
// Index-range ("chunked") rendering, for scenes with more (tile, splat) pairs than one set of lists may hold
// (s2d_sequence.hip chunked_forward / chunked_backward).  The splats are cut into consecutive index ranges; the lists of one range at a time are
// built and walked, front to back like the reference's loops (main.cpp:419, :552), and the per-pixel state is carried
// from range to range in `state` (fp32 whatever the image format): (r, g, b, T).
//   forward pass : raster_forward_chunk_kernel per range; each stores the state and image0 (.w = 1, main.cpp:543-546),
//                  so image0 is final after the last range -- or after the range behind which no pixel is alive any
//                  more (*any_alive stays 0: the host skips the ranges that follow, in both passes).
//   backward pass: raster_backward_chunk_kernel per range, from a fresh state: the forward walk of the range (only for its
//                  hand-over -- the backward walk reads it back, exactly as in the fused kernel) and the backward
//                  walk from the same state, with the FINAL colours of the forward pass out of image0.
// ---------------------------------------------------------------------------------------------------
template <bool HALF, bool EXACT>
__global__ __launch_bounds__(256) void raster_forward_chunk_kernel(const uint32_t* __restrict__ tile_off,
                                                                   const uint32_t* __restrict__ list,
                                                                   const ProjRec* __restrict__ proj, void* __restrict__ image0,
                                                                   float4* __restrict__ state, int first,
                                                                   unsigned long long* __restrict__ wave_masks,
                                                                   uint32_t* __restrict__ exec_list, Geometry g,
                                                                   const DeviceStatus* __restrict__ status, int iteration,
                                                                   uint32_t* __restrict__ any_alive)
{
    __shared__ FwdShared s;
    if (launch_is_void(status, 0, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    float4 st = make_float4(0.0f, 0.0f, 0.0f, 1.0f); // main.cpp:414
    if (!first && c.inside) st = state[pixel_index(c, g)];
    f2 crg = mk2(st.x, st.y);
    float cb = st.z, T = st.w;
    forward_tile<false, EXACT, true>(s, c, tile_off, list, proj, wave_masks, exec_list, nullptr, g, nullptr, crg, cb, &T);
    if (c.inside) {
        state[pixel_index(c, g)] = make_float4(crg.x, crg.y, cb, T);
        store_pixel<HALF>(image0, pixel_index(c, g), make_float4(crg.x, crg.y, cb, 1.0f)); // .w reset, main.cpp:543-546
    }
    if (__ballot(c.inside && !(T < kMinThroughput)) != 0ull && c.lane == 0) atomicOr(any_alive, 1u);
}

template <bool NEED_OP, bool HALF, bool DET, bool EXACT, bool UPSTREAM = false>
__global__ __launch_bounds__(256) void raster_backward_chunk_kernel(const uint32_t* __restrict__ tile_off,
                                                                    const uint32_t* __restrict__ list,
                                                                    const ProjRec* __restrict__ proj,
                                                                    const void* __restrict__ image0,
                                                                    const void* __restrict__ image_ref,
                                                                    float4* __restrict__ state, int first,
                                                                    unsigned long long* __restrict__ wave_masks,
                                                                    uint32_t* __restrict__ exec_list,
                                                                    float* __restrict__ grads, double* __restrict__ tile_sqerr,
                                                                    Geometry g, DetSlots det,
                                                                    const DeviceStatus* __restrict__ status, int iteration)
{
    constexpr size_t kBytes = sizeof(BwdShared<DET>) > sizeof(FwdShared) ? sizeof(BwdShared<DET>) : sizeof(FwdShared);
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
    if (launch_is_void(status, 0, iteration)) return;
    const int tile = tile_of_block(blockIdx.x, g);
    if (tile < 0) return;
    const TileCtx c = tile_ctx(tile, g);
    float4 st = make_float4(0.0f, 0.0f, 0.0f, 1.0f); // image1 = (0,0,0,1), main.cpp:549
    float4 fin = make_float4(0.f, 0.f, 0.f, 0.f), ref = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c.inside) {
        if (!first) st = state[pixel_index(c, g)];
        fin = load_pixel<HALF>(image0, pixel_index(c, g));    // finalColor, main.cpp:613: of ALL ranges
        ref = load_ref_or_upstream<HALF, UPSTREAM>(image_ref, pixel_index(c, g));
    }
    uint32_t n_exec;
    {   // the executed entries of this range, from the state the backward walk starts from (colours discarded)
        f2 crg = mk2(st.x, st.y);
        float cb = st.z, T = st.w;
        n_exec = forward_tile<false, EXACT, true>(*reinterpret_cast<FwdShared*>(smem), c, tile_off, list, proj, wave_masks, exec_list, nullptr, g,
                                                  nullptr, crg, cb, &T);
    }
    __syncthreads(); // as in the fused kernel: LDS re-use, and the hand-over through global memory
    backward_tile<false, NEED_OP, DET, EXACT, true, UPSTREAM>(*reinterpret_cast<BwdShared<DET>*>(smem), c, fin, loss_grad<UPSTREAM>(fin, ref), tile_off, list, proj,
                                                    wave_masks, exec_list, n_exec, grads, tile_sqerr, g, det, nullptr,
                                                    SqerrJob{nullptr, 0, nullptr, nullptr}, &st);
    if (c.inside) state[pixel_index(c, g)] = st;
}

// Deterministic mode: gradient of splat i = sum of the partials its tiles stored this iteration, in emission
// (tile row-major) order -- the same order whatever the dispatch order of the tiles was.  A splat's tiles announce
// themselves in touched[i] (bit j = its j-th emission slot; a tile reaches a splat's entry only while some pixel of it is
// still live, so most of a splat's ~20 slots stay unwritten and a hidden splat has none): the pass reads one word per
// splat and then only the slots that hold something, instead of every stamp of every slot.  Slots from the 32nd on share
// bit 31 and are told apart by their stamps.  The word is cleared for the next pass.
__device__ __forceinline__ void det_add_slot(float (&acc)[9], const float* __restrict__ data, uint32_t slot)
{
    const float4* d = reinterpret_cast<const float4*>(data + (size_t)slot * kDetStride); // three 16-byte loads per slot
    const float4 a = d[0], b = d[1], c = d[2];
    acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
    acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
    acc[8] += c.x;
}

__global__ __launch_bounds__(256) void gather_grads_kernel(const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ counts, int n,
                                                           const float* __restrict__ data,
                                                           const uint32_t* __restrict__ stamp, uint32_t* __restrict__ touched,
                                                           uint32_t now, float* __restrict__ grads)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t m = touched[i];
    if (m == 0u) return; // no tile wrote anything for this splat: its gradient record stays as it is (zero)
    touched[i] = 0u;
    float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const uint32_t o = offsets[i];
    const bool tail = (m >> 31) != 0u;
    m &= 0x7FFFFFFFu;
    while (m != 0u) { // ascending slot order, four slots' loads in flight at a time
        uint32_t js[4];
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (m != 0u) {
                js[q] = (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
                cnt = q + 1;
            }
        float4 v[4][3];
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < cnt) {
                const float4* d = reinterpret_cast<const float4*>(data + (size_t)(o + js[q]) * kDetStride);
                v[q][0] = d[0]; v[q][1] = d[1]; v[q][2] = d[2];
            }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < cnt) {
                acc[0] += v[q][0].x; acc[1] += v[q][0].y; acc[2] += v[q][0].z; acc[3] += v[q][0].w;
                acc[4] += v[q][1].x; acc[5] += v[q][1].y; acc[6] += v[q][1].z; acc[7] += v[q][1].w;
                acc[8] += v[q][2].x;
            }
    }
    if (tail) {
        const uint32_t c = counts[i];
        for (uint32_t s = o + 31u; s < o + c; s++)
            if (stamp[s] == now) det_add_slot(acc, data, s);
    }
    float* gr = grads + (size_t)i * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) gr[k] += acc[k]; // += : the buffer is zero here unless the caller accumulates slabs
}

// Deterministic mode, density statistics: words 9..11 of the same slots, in the same order, into stats[i] (n x 3, accumulated
// over passes).  Runs BEFORE gather_grads_kernel, which clears the `touched` words both read: the statistics ride in the
// gradient slots of their own pass, so a slot is read here exactly when that pass wrote all twelve of its words.
__global__ __launch_bounds__(256) void gather_stats_kernel(const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ counts, int n,
                                                           const float* __restrict__ data,
                                                           const uint32_t* __restrict__ stamp,
                                                           const uint32_t* __restrict__ touched, uint32_t now,
                                                           float* __restrict__ stats)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t m = touched[i];
    if (m == 0u) return;
    float acc[3] = {0.f, 0.f, 0.f};
    const uint32_t o = offsets[i];
    const bool tail = (m >> 31) != 0u;
    m &= 0x7FFFFFFFu;
    while (m != 0u) { // ascending slot order
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        const float4 c = reinterpret_cast<const float4*>(data + (size_t)(o + j) * kDetStride)[2];
        acc[0] += c.y; acc[1] += c.z; acc[2] += c.w;
    }
    if (tail) {
        const uint32_t cnt = counts[i];
        for (uint32_t s = o + 31u; s < o + cnt; s++)
            if (stamp[s] == now) {
                const float4 c = reinterpret_cast<const float4*>(data + (size_t)s * kDetStride)[2];
                acc[0] += c.y; acc[1] += c.z; acc[2] += c.w;
            }
    }
    float* st = stats + (size_t)i * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) st[k] += acc[k];
}

// Sum of the per-tile squared errors in a fixed order (deterministic MSE trace), two stages in one launch:
// kSqerrChunks blocks each reduce a contiguous chunk to partial[b] (sqerr_reduce, s2d_device.h); the block that finishes last (ticket counter)
// adds the partials, again in a fixed order, and re-arms the counter.  scratch = kSqerrChunks doubles + one
// 64-bit counter, zero before the first launch (SqerrTrace, s2d_state.hip, allocates it behind tile_sqerr).
__global__ __launch_bounds__(256) void sqerr_finalize_kernel(const double* __restrict__ tile_sqerr, int num_tiles,
                                                             double* __restrict__ out, double* scratch,
                                                             const DeviceStatus* __restrict__ status, int iteration)
{
    if (status->first_nonfinite_iter < iteration) return;
    sqerr_reduce(tile_sqerr, num_tiles, out, scratch, (int)blockIdx.x, kSqerrChunks);
}

static inline unsigned raster_grid(int num_tiles) { return (unsigned)(((num_tiles + 7) / 8) * 8); }

// Run-time flags -> template arguments: calls f(std::bool_constant<flag>{}...) for the values of (exact, count, half,
// further flags...); a flag given as a std::bool_constant is not branched on.  Which variants exist is decided here and
// nowhere else: exact exp is a validation mode on plain fp32 images without pair counting (s2d_create rejects the
// combinations), so those kernels are never instantiated.  (The order of the flags is the order in which the variants are
// instantiated, which the compiler's register allocation of two counting kernels was seen to depend on: exact goes first.)
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

hipError_t launch_raster(RasterPass pass, const RasterArgs& a, hipStream_t stream)
{
    if (a.g.num_tiles <= 0) return hipSuccess;
    const dim3 grid(raster_grid(a.g.num_tiles)), block(256);
    const DetGather& dg = a.det;
    const bool gather = dg.now != 0u && pass != RasterPass::Forward && pass != RasterPass::ForwardRange;
    const DetSlots det{dg.rects, dg.offsets, dg.data, dg.stamp, dg.touched, dg.now};
    const int first = a.first ? 1 : 0, wi = a.write_image ? 1 : 0;
    const std::false_type no; // a flag the pass has no variants of
    const std::true_type yes;
    hipError_t e = hipErrorInvalidValue;
    const bool stats = a.density != nullptr;
    if (stats) {
        // (dispatched at the end of this function)
    } else if (a.upstream == nullptr) switch (pass) {
    case RasterPass::Forward:
        e = with_variant([&](auto exact, auto count, auto half) {
            hipLaunchKernelGGL((raster_forward_kernel<count, half, exact>), grid, block, 0, stream, a.tile_off, a.list, a.proj,
                               a.image0, a.wave_masks, a.exec_list, a.tile_exec, a.retire_hint, a.g, a.status, a.abort_stamp,
                               a.iteration, a.counters);
        }, a.exact_exp, a.count, a.half_images);
        break;
    case RasterPass::Backward:
        e = with_variant([&](auto exact, auto count, auto half, auto op, auto d) {
            hipLaunchKernelGGL((raster_backward_kernel<count, op, half, d, exact>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, a.image_ref, a.wave_masks, a.exec_list, a.tile_exec, a.grads, a.tile_sqerr, a.g,
                               det, a.status, a.iteration, a.counters);
        }, a.exact_exp, a.count, a.half_images, a.need_opacity_grad, gather);
        break;
    case RasterPass::Fused: // (pair counting is a property of the separate kernels)
        e = with_variant([&](auto exact, auto, auto half, auto op, auto d) {
            hipLaunchKernelGGL((raster_fused_kernel<op, half, d, exact>), grid, block, 0, stream, a.tile_off, a.list, a.proj,
                               a.image0, a.image_ref, a.wave_masks, a.exec_list, a.tile_exec, a.retire_hint, a.grads, a.tile_sqerr,
                               a.g, det, a.status, a.abort_stamp, a.iteration, wi, a.sq);
        }, a.exact_exp, no, a.half_images, a.need_opacity_grad, gather);
        break;
    case RasterPass::ForwardRange:
        e = with_variant([&](auto exact, auto, auto half) {
            hipLaunchKernelGGL((raster_forward_chunk_kernel<half, exact>), grid, block, 0, stream, a.tile_off, a.list, a.proj,
                               a.image0, a.state, first, a.wave_masks, a.exec_list, a.g, a.status, a.iteration, a.any_alive);
        }, a.exact_exp, no, a.half_images);
        break;
    case RasterPass::BackwardRange:
        e = with_variant([&](auto exact, auto, auto half, auto op, auto d) {
            hipLaunchKernelGGL((raster_backward_chunk_kernel<op, half, d, exact>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, a.image_ref, a.state, first, a.wave_masks, a.exec_list, a.grads, a.tile_sqerr,
                               a.g, det, a.status, a.iteration);
        }, a.exact_exp, no, a.half_images, a.need_opacity_grad, gather);
        break;
    }
    // The walks from a caller's loss gradient (a.upstream, in the place of image_ref): the two backward kernels only --
    // a fused launch has no image yet to have a gradient of -- and without pair counting.  Behind everything else on
    // purpose: these instantiations come last, and the kernels above come out of the compiler as they did without them
    // (DESIGN.md section 10).
    else if (a.count) e = hipErrorInvalidValue;
    else if (pass == RasterPass::Backward)
        e = with_variant([&](auto exact, auto, auto half, auto op, auto d, auto up) {
            hipLaunchKernelGGL((raster_backward_kernel<false, op, half, d, exact, up>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, a.upstream, a.wave_masks, a.exec_list, a.tile_exec, a.grads, nullptr, a.g, det,
                               a.status, a.iteration, nullptr);
        }, a.exact_exp, no, a.half_images, a.need_opacity_grad, gather, yes);
    else if (pass == RasterPass::BackwardRange)
        e = with_variant([&](auto exact, auto, auto half, auto op, auto d, auto up) {
            hipLaunchKernelGGL((raster_backward_chunk_kernel<op, half, d, exact, up>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, a.upstream, a.state, first, a.wave_masks, a.exec_list, a.grads, nullptr, a.g, det,
                               a.status, a.iteration);
        }, a.exact_exp, no, a.half_images, a.need_opacity_grad, gather, yes);
    // The density-statistics walk (a.density): the separate backward kernel only, from the reference's loss or a caller's
    // gradient, without pair counting or the exact exponential.  Behind everything else for the same reason as above.
    if (stats && pass == RasterPass::Backward && !a.count && !a.exact_exp)
        e = with_variant([&](auto, auto, auto half, auto op, auto d, auto up, auto st) {
            hipLaunchKernelGGL((raster_backward_kernel<false, op, half, d, false, up, st>), grid, block, 0, stream, a.tile_off, a.list,
                               a.proj, a.image0, up ? (const void*)a.upstream : a.image_ref, a.wave_masks, a.exec_list, a.tile_exec,
                               a.grads, up ? nullptr : a.tile_sqerr, a.g, det, a.status, a.iteration, nullptr,
                               a.density);
        }, no, no, a.half_images, a.need_opacity_grad, gather, a.upstream != nullptr, yes);
    if (e != hipSuccess) return e;
    if (stats && gather && dg.n > 0)
        hipLaunchKernelGGL(gather_stats_kernel, dim3((dg.n + 255) / 256), dim3(256), 0, stream, dg.offsets, dg.counts, dg.n,
                           dg.data, dg.stamp, dg.touched, dg.now, a.density);
    if (gather && dg.n > 0)
        hipLaunchKernelGGL(gather_grads_kernel, dim3((dg.n + 255) / 256), dim3(256), 0, stream, dg.offsets, dg.counts, dg.n,
                           dg.data, dg.stamp, dg.touched, dg.now, a.grads);
    return hipGetLastError();
}

hipError_t launch_sqerr_finalize(SqerrJob sq, const DeviceStatus* status, int iteration, hipStream_t stream)
{
    hipLaunchKernelGGL(sqerr_finalize_kernel, dim3(kSqerrChunks), dim3(256), 0, stream, sq.tile_sqerr, sq.num_tiles, sq.out,
                       sq.scratch, status, iteration);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Reference-order validation mode (S2D_CFG_REFERENCE_ORDER): gradients and squared error bytes-equal
// to the reference's.  Three kernels of their own, behind everything else in this file on purpose: the kernels above come
// out of the compiler as they did without them.  Only order and per-term association differ from
// the fast path; the per-pixel decisions are the forward walk's, taken from its hand-over (exec_list, wave_masks) like
// raster_backward_kernel takes them.  No speed target: no LDS staging, one entry at a time.
// ---------------------------------------------------------------------------------------------------
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
