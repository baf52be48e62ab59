// s2d_walk_backward.h -- the backward walk over a tile's splat list (backward_tile) with its wave sums and LDS layout, and the
// raster_backward_kernel template that the raster units instantiate (s2d_raster.hip: from the target image;
// s2d_raster_gradient.hip: from a caller's gradient, and with density statistics).  Device code, hipcc only.
#pragma once
#include "s2d_walk.h"

namespace s2d {

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
// COVERAGE (S2D_CFG_COVERAGE): the fourth channel is the coverage, its loss the same half squared error -- dL/dA = fin.w - ref.w.
template <bool UPSTREAM, bool COVERAGE = false>
__device__ __forceinline__ float4 loss_grad(const float4 fin, const float4 src)
{
    return UPSTREAM ? src : make_float4(fin.x - src.x, fin.y - src.y, fin.z - src.z, COVERAGE ? fin.w - src.w : 0.0f);
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

// A backward launch's slots: deterministic mode is a.det.now != 0 (the DET kernels), and launch_det_gather follows the walk.
static inline DetSlots det_slots(const DetGather& dg) { return DetSlots{dg.rects, dg.offsets, dg.data, dg.stamp, dg.touched, dg.now}; }

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
// COVERAGE (S2D_CFG_COVERAGE, s2d_raster_coverage.hip): fin.w is the pixel's final coverage and dL.w its loss
// gradient; the walk keeps the running coverage ca beside the colours and the channel sum gets a fourth addend, dL.w * dCa_a with
// dCa_a = T - (fin.w - ca) / (1 - alpha + 1e-15): main.cpp:627-630 for a channel whose colour is 1.  One more running value, one
// more div_by_recip and one more product; everything behind gs, the LDS layout, the wave sums and the flush are untouched.
template <bool COUNT, bool NEED_OP, bool DET, bool EXACT, bool CHUNK = false, bool UPSTREAM = false, bool STATS = false, bool COVERAGE = false>
__device__ __forceinline__ void backward_tile(BwdShared<DET, STATS>& s, const TileCtx& c, const float4 fin, const float4 dL,
                                              const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ list,
                                              const ProjRec* __restrict__ proj,
                                              const unsigned long long* __restrict__ wave_masks,
                                              const uint32_t* __restrict__ exec_list, uint32_t n_handed,
                                              float* __restrict__ grads, double* __restrict__ tile_sqerr,
                                              const Geometry& g, const DetSlots& det, PairCounters* __restrict__ counters,
                                              const SqerrJob& sq, float4* state_io = nullptr, float* __restrict__ stats = nullptr)
{
    static_assert(!(COVERAGE && (COUNT || EXACT || CHUNK || STATS)), "the coverage channel: plain lists, exp_approx, no counting, no statistics");
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
    [[maybe_unused]] float ca = 0.0f;
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
                    if constexpr (COVERAGE) ca += T * alpha;                         // the same with c = 1
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
                    float gs = (pr.x + pr.y) + dLb * dCa_b;
                    if constexpr (COVERAGE) gs = gs + dL.w * (T - div_by_recip(fin.w - ca, den, rd)); // + dLa * dCa_a
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

} // namespace s2d
