// s2d_api.hip -- the C ABI of include/splat2d.h: context, device memory, iteration sequencing.
//
// One iteration (main.cpp:414-809) of s2d_step is TWO launches on the context's stream:
//   raster_fused (forward walk + backward walk + per-tile squared error of every tile)
//   -> adam (+ the sum of the tile errors, + projection of the updated splats and the containment check for the next
//      iteration)
// s2d_forward / s2d_backward / s2d_adam_step queue the passes one by one (raster_forward, raster_backward, sqerr_finalize).
// When the tile lists have to be (re)built:  project -> TileLists (s2d_lists.h): count scan -> emit -> sort -> tile offsets.
// The host never makes the GPU wait: it reads the 4-byte containment flag after launching the raster kernel
// optimistically, and the 4-byte pair count only when lists are rebuilt.
#include "../../include/splat2d.h"
#include "../../include/splat2d_test.h"

#include <algorithm>
#include <vector>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>

#include "s2d_device.h"
#include "s2d_context.h"
#include "s2d_density.h" // (behind s2d_device.h: s2d_math.h's qualifiers need the HIP runtime header under hipcc)
#include "s2d_lists.h"
#include "s2d_loss.h"
#include "s2d_owned.h"
#include "s2d_seed.h"
#include "s2d_seed_math.h"
#include "s2d_state.h"

using namespace s2d;

struct s2d_ctx {
    s2d_config cfg{};
    Geometry g{};
    int n = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    float lr = 0.05f;

    SplatState state;            // parameters, optimiser state, the held set of slab ownership (s2d_state.h)
    DevBuf<float> d_grads_own;   // gradients (AoS, the reference's layout)
    float* d_grads = nullptr;    // buffer in use (own or bound)
    // projection + binning
    DevBuf<ProjRec> d_proj;
    DevBuf<TileRect> d_rects;
    DevBuf<uint32_t> d_counts;
    DevBuf<uint32_t> d_offsets;
    DevBuf<uint32_t> d_scan_temp;               // lent to the list builds and to s2d_halo_commit
    TileLists lists;                            // the per-tile lists and everything only their builds use
    PairScratch scratch;                        // the raster's hand-over and slots, sized like the lists (s2d_context.h)
    IndexRanges ranges;                         // scenes beyond one set of lists: the cut, the carry, the progress of a pass
    bool lists_valid = false;
    bool proj_fresh = false; // d_proj and d_status->rebin_needed describe the CURRENT parameters
    ListReuse reuse;         // when lists are rebuilt on schedule, and the stamped containment check (s2d_context.h)
    // images
    // image0 / imageRef (main.cpp:310, :254): the rows [row_begin, row_end) of this context's slab only -- a context
    // never touches another row, so a 1/8 slab of 8192^2 holds 2 x 134 MB instead of 2 x 1.07 GB
    DevBuf<uint8_t> d_image0;  // bytes: RGBA32F, or 4 x fp16 per pixel with S2D_CFG_FP16_IMAGES
    DevBuf<uint8_t> d_ref;
    bool half_images = false;
    size_t pixel_bytes = sizeof(float4);
    SqerrTrace trace;          // the tile errors of a backward pass and the ring of per-iteration sums (s2d_state.h)
    DensityStats density;      // what the passes with S2D_BWD_DENSITY_STATS accumulated (s2d_state.h)
    // loss passes (s2d_loss_*, s2d_loss.h): everything here is allocated by the first call that needs it
    LossTrace loss;                // per-tile sums and the ring of per-iteration totals
    DevBuf<float> d_loss_maps;     // [9][pixels]: the derivative maps between the two window passes (w_dssim > 0 only)
    DevBuf<float4> d_loss_grad;    // dL/d(image0) of s2d_loss_backward / s2d_step_loss
    SeedScratch seed;              // the importance map of s2d_importance / s2d_seed_splats / s2d_reseed (s2d_seed.h), on first use
    DevBuf<DeviceStatus> d_status;
    DevBuf<PairCounters> d_counters;
    // pinned host mirrors
    HostBuf<DeviceStatus> h_status;

    // host-side state of the reference's main()
    float beta1t = 1.0f, beta2t = 1.0f; // main.cpp:274-275
    int iterations = 0;                 // main.cpp:278
    float good_beta1t = 1.0f, good_beta2t = 1.0f; // the three above at the last point known to be finite
    int good_iterations = 0;
    bool have_target = false;
    bool have_forward = false;  // image0 holds the framebuffer of the CURRENT parameters (s2d_backward reads it)
    bool have_backward = false;
    char err[512] = {0};
    S2D_LOCAL ~s2d_ctx() = default; // (named only to keep it out of the library's exports, like the owners it runs)
};

namespace {

int fail(s2d_ctx* c, int code, const char* fmt, ...)
{
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof(c->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define S2D_HIP(c, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail((c), S2D_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Declared behind a temporary device buffer that work queued on `stream` uses: the stream is idle before the buffer
// is freed, on whichever way the function is left.
struct IdleAtExit {
    hipStream_t stream;
    ~IdleAtExit() { (void)hipStreamSynchronize(stream); }
};

int use_device(s2d_ctx* c)
{
    S2D_HIP(c, hipSetDevice(c->device));
    return S2D_OK;
}

// The single place where pair capacity grows: the pair buffers of the lists and the raster's scratch have one size.
// Every one of them is released, with the stream idle, before the first is allocated again.
int ensure_pair_capacity(s2d_ctx* c, uint64_t need)
{
    if (need <= c->lists.capacity()) return S2D_OK;
    if (need >= 0xFFFF0000ull) return fail(c, S2D_E_NOMEM, "tile lists need %llu pairs (> 2^32)", (unsigned long long)need);
    uint64_t cap = std::max<uint64_t>(need + need / 4 + 4096, 1 << 16);
    if (cap > 0xFFFF0000ull) cap = 0xFFFF0000ull;
    const PairScratch::Grant grant = c->scratch.admit(need, cap); // refused before anything is released or launched
    if (!grant.slots)
        return fail(c, S2D_E_NOMEM, "the term scratch of S2D_CFG_REFERENCE_ORDER needs %llu bytes for %llu (tile, splat) pairs, "
                    "S2D_REFERENCE_ORDER_MAX_BYTES allows %llu", (unsigned long long)grant.bytes, (unsigned long long)grant.refused,
                    (unsigned long long)c->scratch.max_bytes());
    cap = grant.slots;
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    c->lists.release_pairs();
    c->scratch.release();
    S2D_HIP(c, c->lists.alloc_pairs(cap));
    const hipError_t scratch_alloc = c->scratch.alloc(cap);
    if (scratch_alloc != hipSuccess) c->lists.release_pairs(); // (capacity 0 is what is left if an allocation fails)
    S2D_HIP(c, scratch_alloc);
    return S2D_OK;
}

// (Re)build the per-tile lists from the current parameters.  The projection has already been queued with mode 0.
// first / count: the index range of the splats to list (count < 0: all of them).  A range's lists hold indices RELATIVE to
// its first splat -- every per-splat array is handed over from that splat on -- and so do the scanned offsets.
// *need_ranges (all splats only): their pairs exceed the budget of one set of lists, nothing was built.
int rebuild_lists(s2d_ctx* c, int first = 0, int count = -1, bool* need_ranges = nullptr)
{
    const int n = count < 0 ? c->n : count;
    uint64_t total = 0;
    c->lists_valid = false; // (count() already writes into the buffers the lists lie in)
    S2D_HIP(c, c->lists.count(ListInput{c->d_rects + first, c->d_counts + first, c->d_offsets + first, first, n, c->d_scan_temp},
                              c->stream, &total));
    if (need_ranges) *need_ranges = total > c->ranges.budget();
    if (need_ranges && *need_ranges) return S2D_OK;
    if (total >= 0xFFFF0000ull)
        return fail(c, S2D_E_NOMEM, "the tile lists of splats %d..%d need more than 2^32 - 65536 (tile, splat) pairs", first, first + n - 1);
    if (int rc = ensure_pair_capacity(c, total)) return rc;
    S2D_HIP(c, c->lists.finish(c->stream));
    c->lists_valid = count < 0; // a range's lists are walked once and replaced by the next range's
    return S2D_OK;
}

// What a raster pass of the context works on: the lists of all splats, or (range >= 0) those of one index range.  A
// range's lists hold indices relative to its first splat, so every per-splat array is handed over from that splat on.
RasterArgs raster_args(const s2d_ctx* c, int range = -1)
{
    const int first = range < 0 ? 0 : c->ranges.first(range), count = range < 0 ? c->n : c->ranges.size(range);
    RasterArgs a;
    a.tile_off = c->lists.tile_off(); a.list = c->lists.list();
    a.proj = c->d_proj + first; a.grads = c->d_grads + (size_t)first * 9;
    a.image0 = c->d_image0; a.image_ref = c->d_ref; a.tile_sqerr = c->trace.tile_sqerr();
    a.g = c->g; a.status = c->d_status; a.iteration = c->iterations; a.counters = c->d_counters;
    c->scratch.fill(&a, c->d_rects, c->d_offsets, c->d_counts, first, count);
    c->ranges.fill(&a, range);
    a.half_images = c->half_images; a.count = (c->cfg.flags & S2D_CFG_COUNT_PAIRS) != 0; a.exact_exp = (c->cfg.flags & S2D_CFG_EXACT_EXP) != 0;
    return a;
}

// What a projection pass works on.  check == nullptr (mode 0): rectangles (inflated by the re-use margin), pair and row
// counts for a list build; otherwise (mode 1): that containment check against those rectangles.
ProjectArgs project_args(const s2d_ctx* c, const float* splats, const ContainmentCheck* check)
{
    ProjectArgs a;
    a.splats = splats; a.held = c->state.held(); a.n = c->n; a.g = c->g; a.mode = check ? 1 : 0; a.proj = c->d_proj; a.counts = c->d_counts;
    a.check = check ? *check : ContainmentCheck{c->d_rects, c->d_status};
    if (!check) a.margin = c->reuse.margin(), a.row_counts = c->lists.row_counts();
    return a;
}

// What an Adam launch works on.  project: the kernel also projects what it wrote and runs the containment check.
AdamArgs adam_args(s2d_ctx* c, uint32_t flags, bool project)
{
    const SplatState::AdamStep st = c->state.adam_step();
    AdamArgs a;
    a.splats = st.arrays.splats; a.adams = st.arrays.adams; a.grads = c->d_grads; a.compact = st.compact;
    a.held_ids = st.held_ids; a.held_count = st.held_count; a.dormant = st.dormant; a.n = c->n; a.g = c->g;
    a.beta1t = c->beta1t; a.beta2t = c->beta2t; a.lr = c->lr; a.iteration = c->iterations;
    a.mode = ((flags & S2D_STEP_OPTIMIZE_OPACITY) ? 1 : 0) | ((c->cfg.flags & S2D_CFG_ADAM_FP32) ? 2 : 0);
    a.proj = project ? (ProjRec*)c->d_proj : nullptr;
    a.proj_current = c->proj_fresh; // (every event that replaces parameters clears it: invalidate())
    a.check = project ? c->reuse.next_check(c->d_rects, c->d_status) : c->reuse.idle_check(c->d_rects, c->d_status);
    a.sq = c->trace.take_for_adam();
    return a;
}

// The pass has a backward walk (deterministic mode: with a fresh stamp for its slots).
void with_backward_walk(s2d_ctx* c, RasterArgs& a, bool need_opacity_grad) { a.need_opacity_grad = need_opacity_grad, c->scratch.backward_walk(&a); }

// ---------------------------------------------------------------------------------------------------------------------
// Index-range ("chunked") rendering.  The reference's loops have no limit on the number of (pixel, splat) pairs
// (main.cpp:492-536); 32-bit list positions have one, and long before it the list and mask buffers have a price.  A scene
// beyond the budget of IndexRanges is rendered range by range: cut where the running pair count would pass the budget,
// build the lists of one range, walk them, carry the per-pixel (colour, T) to the next range.  Blend order is index order
// (main.cpp:419), so the cut changes no operation: the framebuffer is bit for bit the unchunked one, and so is every
// gradient term (the sums differ in the order the atomics arrive, as always).  Lists are rebuilt every pass: this is the
// path for scenes that do not fit, not a fast one.
// ---------------------------------------------------------------------------------------------------------------------
// The lists of range k (built unless the buffers hold them already), and what a raster pass over them works on.
int build_chunk(s2d_ctx* c, int k, RasterArgs* a)
{
    if (!c->ranges.built(k)) {
        c->ranges.set_built(-1);
        if (int rc = rebuild_lists(c, c->ranges.first(k), c->ranges.size(k))) return rc;
        c->ranges.set_built(k);
    }
    *a = raster_args(c, k);
    return S2D_OK;
}

// Forward pass over the ranges (main.cpp:414-546); stops behind the range after which no pixel of the slab is above the
// throughput cut-off any more (main.cpp:520: nothing later could change a pixel).
int chunked_forward(s2d_ctx* c)
{
    const int K = c->ranges.count();
    c->ranges.begin_forward();
    for (int k = 0; k < K; k++) {
        RasterArgs a;
        if (int rc = build_chunk(c, k, &a)) return rc;
        S2D_HIP(c, c->ranges.launching_forward(k));
        S2D_HIP(c, launch_raster(RasterPass::ForwardRange, a, c->stream));
        bool alive = true;
        if (k + 1 < K) S2D_HIP(c, c->ranges.any_alive(&alive));
        if (!alive) break;
    }
    return S2D_OK;
}

// Backward pass over the same ranges (main.cpp:548-712), from a fresh per-pixel state; image0 holds the final colours.
// upstream: as in queue_backward.
int chunked_backward(s2d_ctx* c, bool need_opacity_grad, const float4* upstream = nullptr)
{
    for (int k = 0; k < c->ranges.walked(); k++) {
        RasterArgs a;
        if (int rc = build_chunk(c, k, &a)) return rc;
        a.upstream = upstream;
        with_backward_walk(c, a, need_opacity_grad);
        S2D_HIP(c, launch_raster(RasterPass::BackwardRange, a, c->stream));
    }
    return S2D_OK;
}

// First raster launch of an iteration, on lists believed (optimistic) or known to cover the current parameters:
// the forward kernel alone, or the fused forward + backward kernel.
struct RasterJob {
    bool fused = false;        // forward + backward walk in one launch
    bool need_opacity_grad = true;
    bool write_image = true;   // fused only: store image0 (nothing but s2d_get_image reads it)
};

int launch_job(s2d_ctx* c, bool optimistic, const RasterJob& job)
{
    RasterArgs a = raster_args(c);
    a.abort_stamp = optimistic ? c->reuse.abort_stamp() : 0;
    if (job.fused) {
        with_backward_walk(c, a, job.need_opacity_grad);
        a.write_image = job.write_image;
        if (c->trace.plan(true, true) == SqerrBy::PassItself) a.sq = c->trace.job(c->iterations);
    }
    if (c->scratch.reference_order() && a.exact_exp) // (never fused: queue_forward_backward)
        S2D_HIP(c, launch_reference_forward_exact(a, c->stream));
    else
        S2D_HIP(c, launch_raster(job.fused ? RasterPass::Fused : RasterPass::Forward, a, c->stream));
    return S2D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// What is current, and what makes it stale.  Three things are derived from the parameters, each from the one before:
// the projection with its containment check (proj_fresh), the tile lists (lists_valid), and the frames -- image0 and
// the gradients (have_forward, have_backward).  The functions that produce them set these flags (rebuild_lists,
// queue_raster, backward_queued, queue_adam); everything else names an event, and invalidate()
// clears what the event reaches: Frames < Projection < Lists, a level with everything below it.
//   target replaced (s2d_set_target, _synthetic): Frames.
//   all splats replaced (s2d_init_splats, s2d_set_splats): Lists; splats_replaced() = state.written() + a fresh status
//     word.  init also zeroes the gradients and restarts the counters, and asks for the arrays with discard_all(): every
//     record, moments included, is new.
//   some splat rows replaced (s2d_rows_scatter; s2d_relocate, s2d_seed_splats, s2d_reseed): Projection; state.written().  Not Lists: a row moves a splat a little,
//     and the containment check of the projection that follows asks for new lists if it left its rectangle.
//   all splats replaced from device memory (s2d_set_splats_device): as some rows, over all of them -- Projection;
//     state.written().  Not Lists, and no fresh status word: this is the call of an optimisation loop outside the
//     library, which moves every splat a little per call; a splat that left its rectangle gets its new lists from the
//     same containment check.
//   moments replaced (s2d_set_adam, s2d_rows_scatter): nothing, what is drawn depends on the parameters only; state.written().
//   held set changed (s2d_halo_commit): Lists if splats arrived, on the first commit and on the return to holding
//     everything (the lists hold the held splats only); departures alone leave lists that still cover every held splat.
//   Adam step queued (queue_adam): Projection, which the step itself renews when it projects (ListReuse::adam_checks).
//     The launch is told proj_fresh as it stands BEFORE the step: only then may it leave the record and the check of a
//     splat it does not move as they are (adam_kernel); after any of the events above it projects and checks every splat.
//   non-finite step judged (judge_status): Frames; the counters are wound back to the failing step.
//   index-range pass finished (queue_raster): the last range's lists are no lists of the scene, lists_valid stays false.
// Rules that are not in this table because no call site keeps them any more.  s2d_state.h: the id-indexed parameter and
// moment arrays are handed out by SplatState::current() only, which queues the write-back of a compact copy first; and a
// squared-error sum still waiting for its Adam launch is queued by SqerrTrace's own read() and settle(), the latter
// being what s2d_set_adam and s2d_init_splats call before they renumber the iterations.  s2d_context.h: a stamp that asked
// for new lists matches nothing once they are built, and every containment check has a sequence number of its own
// (ListReuse); the slots of an earlier backward walk are invalid in the next (PairScratch); which range's lists are in
// the buffers, and how far the last forward pass over ranges got (IndexRanges).
// ---------------------------------------------------------------------------------------------------------------------
enum class Stale { Frames, Projection, Lists };

void invalidate(s2d_ctx* c, Stale reach)
{
    c->have_forward = c->have_backward = false;
    if (reach >= Stale::Projection) c->proj_fresh = false;
    if (reach >= Stale::Lists) c->lists_valid = false;
}

constexpr DeviceStatus kFreshStatus{0, INT_MAX, 0, 0}; // rebin_needed 0 matches no check (sequence numbers start at 1)

// New parameters (init / set_splats): a non-finite event of the old ones no longer stops the queue.
int splats_replaced(s2d_ctx* c)
{
    S2D_HIP(c, c->state.written(true));
    S2D_HIP(c, hipMemcpyAsync(c->d_status, &kFreshStatus, sizeof(DeviceStatus), hipMemcpyHostToDevice, c->stream));
    invalidate(c, Stale::Lists);
    return S2D_OK;
}

// Project the splats, make sure the tile lists cover them, run the forward raster (or the fused forward + backward).
//
// Steady state (lists re-used): the projection of the current parameters and the containment check were produced by
// the Adam kernel of the previous iteration, which stamps a device word and a host-mapped word with the check's
// sequence number if some splat left its binned rectangle.  The raster kernel is launched OPTIMISTICALLY: it
// compares the device word with that sequence number and does nothing on a match, and the host reads its word only
// after the launch (waiting for the CHECKING kernel, not the raster kernel), so the GPU never waits for the host and
// no flag has to be copied or cleared.  If the check failed the lists are rebuilt and the raster kernel is
// launched again.  (In deterministic mode the gather pass queued behind a voided fused launch adds nothing: the
// slots carry no stamp of that pass.)
int queue_project(s2d_ctx* c, const ContainmentCheck* check = nullptr)
{
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, launch_project(project_args(c, now.splats, check), c->stream));
    return S2D_OK;
}

int queue_raster(s2d_ctx* c, const RasterJob& job)
{
    if (!c->have_target) return fail(c, S2D_E_STATE, "no target image set (s2d_set_target)");
    const bool scheduled = c->reuse.rebuild_scheduled(c->lists_valid);
    bool rebuild = scheduled;
    bool stored_image0 = !job.fused || job.write_image; // a fused launch told not to store image0 leaves an older frame there
    if (!scheduled) {
        if (!c->proj_fresh) { // parameters changed without a fused projection: project + check now
            const ContainmentCheck check = c->reuse.next_check(c->d_rects, c->d_status);
            if (int rc = queue_project(c, &check)) return rc;
            S2D_HIP(c, c->reuse.check_queued());
            c->proj_fresh = true;
        }
        if (int rc = launch_job(c, true, job)) return rc;
        S2D_HIP(c, c->reuse.asked_for_lists(&rebuild)); // (waits for the checking kernel, not the raster kernel)
    }
    if (rebuild) {
        int rc = queue_project(c);
        if (rc != S2D_OK) return rc;
        c->ranges.clear();
        bool need_ranges = false;
        if ((rc = rebuild_lists(c, 0, -1, &need_ranges)) != S2D_OK) return rc;
        if (need_ranges && (c->cfg.flags & S2D_CFG_COUNT_PAIRS))
            return fail(c, S2D_E_NOMEM, "pair counting (S2D_CFG_COUNT_PAIRS) is not available for scenes beyond %llu (tile, splat) pairs",
                        (unsigned long long)c->ranges.budget());
        if (need_ranges && c->scratch.reference_order())
            return fail(c, S2D_E_NOMEM, "reference order (S2D_CFG_REFERENCE_ORDER) is not available for scenes beyond %llu (tile, splat) pairs",
                        (unsigned long long)c->ranges.budget());
        c->proj_fresh = true;
        c->reuse.lists_rebuilt();
        if (need_ranges) {
            // more pairs than one set of lists may hold: render by index ranges (every pass rebuilds: lists_valid stays false)
            S2D_HIP(c, c->ranges.plan(c->d_counts, c->n));
            if ((rc = chunked_forward(c)) != S2D_OK) return rc;
            if (job.fused && (rc = chunked_backward(c, job.need_opacity_grad)) != S2D_OK) return rc;
            stored_image0 = true; // the forward pass over the ranges always stores it
        } else if ((rc = launch_job(c, false, job)) != S2D_OK) {
            return rc;
        }
    }
    c->have_forward = stored_image0;
    c->have_backward = false;
    return S2D_OK;
}

int queue_forward(s2d_ctx* c) { return queue_raster(c, RasterJob{}); }

// A backward pass of the current iteration has been queued; `by`: what becomes of its squared error (SqerrTrace::plan,
// or what the pass has done about it already).
int backward_queued(s2d_ctx* c, SqerrBy by)
{
    c->have_backward = true;
    S2D_HIP(c, c->trace.record(c->iterations, by));
    return S2D_OK;
}

// S2D_CFG_REFERENCE_ORDER: terms into their slots, the ordered sums into the gradient buffer, and the squared error as one
// ordered chain straight into the ring slot -- nothing is left to the Adam launch.  (Such a context never renders by
// index ranges, queue_raster refuses the scene, and holds every splat: the state's write-back is a no-op.)
int queue_backward_reference(s2d_ctx* c, bool need_opacity_grad, const float4* upstream)
{
    RasterArgs a = raster_args(c);
    a.upstream = upstream;
    a.need_opacity_grad = need_opacity_grad;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    const RefOrder ro = c->scratch.reference_walk(now.splats, c->d_rects, c->d_offsets, c->d_counts, c->n);
    S2D_HIP(c, launch_reference_backward(a, ro, c->stream));
    if (upstream) return backward_queued(c, SqerrBy::NoLoss);
    S2D_HIP(c, launch_reference_sqerr(c->scratch.pixel_sqerr(), (size_t)c->g.W * (size_t)(c->g.row_end - c->g.row_begin),
                                      c->trace.job(c->iterations).out, c->d_status, c->iterations, c->stream));
    return backward_queued(c, SqerrBy::PassItself);
}

// What the flags of a backward pass (S2D_BWD_*) or of a step (step: S2D_STEP_*) ask of the backward walk.  The density
// statistics are refused here for a context whose configuration has no such walk (the STATS kernels exist without pair
// counting and the exact exponential; reference order has kernels of its own).
struct WalkFlags {
    bool need_opacity_grad = true;
    bool density = false;
};

int parse_walk_flags(s2d_ctx* c, uint32_t flags, bool step, WalkFlags* out)
{
    out->need_opacity_grad = step ? (flags & S2D_STEP_OPTIMIZE_OPACITY) != 0 : !(flags & S2D_BWD_SKIP_OPACITY_GRAD);
    out->density = (flags & (step ? S2D_STEP_DENSITY_STATS : S2D_BWD_DENSITY_STATS)) != 0;
    if (out->density && ((c->cfg.flags & (S2D_CFG_COUNT_PAIRS | S2D_CFG_EXACT_EXP)) || c->scratch.reference_order()))
        return fail(c, S2D_E_INVALID, "density statistics are not available with S2D_CFG_COUNT_PAIRS, S2D_CFG_EXACT_EXP or "
                    "S2D_CFG_REFERENCE_ORDER");
    return S2D_OK;
}

// upstream != nullptr (s2d_backward_image_grads): the walk starts from the caller's dL/d(image0) instead of
// image0 - imageRef.  The loss is the caller's, so no squared error is formed or queued: the trace ring and a sum still
// waiting for the next Adam launch stay as the last s2d_backward left them (SqerrBy::NoLoss).
// density (S2D_BWD_DENSITY_STATS; parse_walk_flags() has admitted it): the walk also accumulates the density statistics.
int queue_backward(s2d_ctx* c, bool need_opacity_grad, const float4* upstream = nullptr, bool density = false)
{
    if (!c->have_forward) return fail(c, S2D_E_STATE, "the backward pass needs s2d_forward on the current parameters");
    if (c->scratch.reference_order()) return queue_backward_reference(c, need_opacity_grad, upstream);
    if (density && c->ranges.active())
        return fail(c, S2D_E_NOMEM, "density statistics are not available for scenes beyond %llu (tile, splat) pairs (index-range rendering)",
                    (unsigned long long)c->ranges.budget());
    if (c->ranges.active()) { // the forward pass went over index ranges: so does this one
        if (int rc = chunked_backward(c, need_opacity_grad, upstream)) return rc;
    } else {
        RasterArgs a = raster_args(c);
        a.upstream = upstream;
        if (density) S2D_HIP(c, c->density.next_pass(&a.density));
        with_backward_walk(c, a, need_opacity_grad);
        S2D_HIP(c, launch_raster(RasterPass::Backward, a, c->stream));
    }
    return backward_queued(c, upstream ? SqerrBy::NoLoss : c->trace.plan(false, false));
}

// Forward + backward (+ squared error) of the current parameters through the fused kernel.  Pair counting is a
// property of the separate kernels only, so a counting context takes those.
int queue_forward_backward(s2d_ctx* c, bool need_opacity_grad, bool write_image)
{
    if ((c->cfg.flags & S2D_CFG_COUNT_PAIRS) || c->scratch.reference_order()) { // (reference order: its backward pass is a launch of its own)
        if (int rc = queue_forward(c)) return rc;
        return queue_backward(c, need_opacity_grad);
    }
    RasterJob job;
    job.fused = true;
    job.need_opacity_grad = need_opacity_grad;
    job.write_image = write_image;
    if (int rc = queue_raster(c, job)) return rc;
    return backward_queued(c, c->trace.plan(true, !c->ranges.active())); // (launch_job asked the same plan about the fused launch)
}

int queue_adam(s2d_ctx* c, uint32_t flags)
{
    c->beta1t *= kAdamBeta1; // main.cpp:718-719
    c->beta2t *= kAdamBeta2;
    // With re-usable lists the Adam kernel also projects the updated splats and checks them against their binned
    // rectangles (what the next forward needs), which saves a pass over the parameters per iteration.
    const bool fuse = c->reuse.adam_checks(c->lists_valid);
    S2D_HIP(c, launch_adam(adam_args(c, flags, fuse), c->stream));
    if (fuse) S2D_HIP(c, c->reuse.check_queued());
    invalidate(c, Stale::Projection);
    c->proj_fresh = fuse; // (then the step projected what it wrote)
    c->iterations++; // main.cpp:809
    c->reuse.step_queued();
    return S2D_OK;
}

int queue_status_read(s2d_ctx* c) // -> h_status, valid once the stream has been synchronised
{
    S2D_HIP(c, hipMemcpyAsync(c->h_status, c->d_status, sizeof(DeviceStatus), hipMemcpyDeviceToHost, c->stream));
    return S2D_OK;
}

// The status word has been copied to h_status and the stream synchronised: act on it.
int judge_status(s2d_ctx* c)
{
    if (c->h_status->nonfinite) {
        // The kernels queued behind the failing Adam step did nothing: put the host-side counters back to where the
        // device stopped (that step's update is the last thing that happened, as at the reference's abort()).
        const int k = c->h_status->first_nonfinite_iter;
        if (k >= c->good_iterations && k < c->iterations) {
            float b1 = c->good_beta1t, b2 = c->good_beta2t;
            for (int i = c->good_iterations; i <= k; i++) { b1 *= kAdamBeta1; b2 *= kAdamBeta2; } // main.cpp:718-719
            c->beta1t = b1;
            c->beta2t = b2;
            c->iterations = k + 1;
            invalidate(c, Stale::Frames);
        }
        return fail(c, S2D_E_NONFINITE, "non-finite parameter after iteration %d (the reference abort()s, main.cpp:752-785)", k);
    }
    c->good_beta1t = c->beta1t;
    c->good_beta2t = c->beta2t;
    c->good_iterations = c->iterations;
    return S2D_OK;
}

int check_status(s2d_ctx* c)
{
    if (int rc = queue_status_read(c)) return rc;
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return judge_status(c);
}

double mse_norm(const s2d_ctx* c) { return (double)((long long)c->g.H * c->g.W * 3); }

size_t slab_pixels(const s2d_ctx* c) { return (size_t)c->g.W * (size_t)(c->g.row_end - c->g.row_begin); }

// ---- loss passes (s2d_loss.h) --------------------------------------------------------------------------------------
// Everything s2d_loss_* refuses for the configuration or the context, before any device work.
int loss_refused(s2d_ctx* c, const s2d_loss_config* cfg)
{
    if (!cfg || cfg->struct_size != sizeof(s2d_loss_config)) return fail(c, S2D_E_INVALID, "s2d_loss_config: NULL or wrong struct_size");
    const float w[3] = {cfg->w_mse, cfg->w_l1, cfg->w_dssim};
    for (float v : w)
        if (!(v >= 0.0f) || std::isinf(v)) return fail(c, S2D_E_INVALID, "loss weights must be finite and >= 0");
    if (w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f) return fail(c, S2D_E_INVALID, "all loss weights are zero");
    if (c->g.row_begin != 0 || c->g.row_end != c->g.H)
        return fail(c, S2D_E_INVALID, "the loss window crosses slab rows: this context owns a row slab");
    if (c->state.held()) return fail(c, S2D_E_INVALID, "the loss passes need every splat: this context holds a subset (s2d_halo_commit)");
    if (c->cfg.flags & S2D_CFG_COUNT_PAIRS)
        return fail(c, S2D_E_INVALID, "pair counting (S2D_CFG_COUNT_PAIRS) has no backward pass from an image gradient");
    return S2D_OK;
}

// The loss kernels of the current frame: dL/d(image0) -> dimage, the totals -> `slot` of the loss ring, the squared error
// also -> sqerr_out (the iteration's slot of the squared-error ring, or null).
int queue_loss(s2d_ctx* c, const s2d_loss_config* cfg, float4* dimage, int slot, double* sqerr_out)
{
    if (!c->have_forward) return fail(c, S2D_E_STATE, "the loss needs s2d_forward on the current parameters");
    S2D_HIP(c, c->loss.ensure(c->g.W, c->g.H, c->stream));
    if (cfg->w_dssim > 0.0f && !c->d_loss_maps) S2D_HIP(c, c->d_loss_maps.alloc((size_t)kLossMapPlanes * slab_pixels(c)));
    LossArgs a;
    a.image0 = c->d_image0; a.image_ref = c->d_ref; a.half_images = c->half_images; a.W = c->g.W; a.H = c->g.H;
    a.w_mse = cfg->w_mse; a.w_l1 = cfg->w_l1; a.w_dssim = cfg->w_dssim;
    a.maps = c->d_loss_maps; a.dimage = dimage; a.partial = c->loss.partial(); a.out3 = c->loss.slot(slot); a.sqerr_out = sqerr_out;
    a.status = c->d_status; a.iteration = c->iterations;
    S2D_HIP(c, launch_loss(a, c->stream));
    c->loss.record(slot, cfg->w_mse, cfg->w_l1, cfg->w_dssim);
    return S2D_OK;
}

// s2d_backward for the loss: the loss kernels into the context's gradient image, the backward walk from it, and the
// squared error of the iteration in the ring as the loss finalize left it (SqerrBy::LossPass).
int queue_loss_backward(s2d_ctx* c, const s2d_loss_config* cfg, bool need_opacity_grad, bool density)
{
    if (!c->have_forward) return fail(c, S2D_E_STATE, "the backward pass needs s2d_forward on the current parameters");
    if (!c->d_loss_grad) S2D_HIP(c, c->d_loss_grad.alloc(slab_pixels(c)));
    if (int rc = queue_loss(c, cfg, c->d_loss_grad, LossTrace::slot_of(c->iterations), c->trace.job(c->iterations).out)) return rc;
    if (int rc = queue_backward(c, need_opacity_grad, c->d_loss_grad, density)) return rc;
    return backward_queued(c, SqerrBy::LossPass);
}

// Sums of a loss pass (squared error on the 255 scale, |d|, 1 - s) -> the means and the total; a term with weight 0 was not formed.
s2d_loss_terms loss_terms_of(const s2d_ctx* c, const double* sums, const float* w)
{
    const double n3 = mse_norm(c);
    s2d_loss_terms t;
    t.mse = sums[0] / (255.0 * 255.0) / n3;
    t.l1 = w[1] > 0.0f ? sums[1] / n3 : std::nan("");
    t.dssim = w[2] > 0.0f ? sums[2] / n3 : std::nan("");
    t.total = 0.0;
    if (w[0] > 0.0f) t.total += (double)w[0] * 0.5 * t.mse;
    if (w[1] > 0.0f) t.total += (double)w[1] * t.l1;
    if (w[2] > 0.0f) t.total += (double)w[2] * t.dssim;
    return t;
}

// The image crosses the ABI as floats; a context with S2D_CFG_FP16_IMAGES keeps halves (round to nearest even) and
// converts on the way, through a temporary where the other side is host memory.
// The whole target (main.cpp:254-259) -> imageRef; a slab context uploads and keeps its own rows only.  Waits.
int upload_target(s2d_ctx* c, const float* rgba32f)
{
    const size_t px = slab_pixels(c), bytes = px * sizeof(float4);
    const float* src = rgba32f + (size_t)c->g.row_begin * c->g.W * 4;
    if (c->half_images) {
        DevBuf<float4> tmp;
        S2D_HIP(c, tmp.alloc(px));
        const IdleAtExit idle{c->stream}; // (before tmp goes)
        S2D_HIP(c, hipMemcpyAsync(tmp, src, bytes, hipMemcpyHostToDevice, c->stream));
        S2D_HIP(c, launch_convert_f32_to_f16(tmp, c->d_ref, px, c->stream));
    } else {
        S2D_HIP(c, hipMemcpyAsync(c->d_ref, src, bytes, hipMemcpyHostToDevice, c->stream));
    }
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

// image0 (the rows of the slab) -> dst.  to_host: waits; otherwise dst is device memory and the copy is only queued.
int download_image0(s2d_ctx* c, float* dst, bool to_host)
{
    const size_t px = slab_pixels(c), bytes = px * sizeof(float4);
    if (!c->half_images) {
        S2D_HIP(c, hipMemcpyAsync(dst, c->d_image0, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    } else if (!to_host) {
        S2D_HIP(c, launch_convert_f16_to_f32(c->d_image0, reinterpret_cast<float4*>(dst), px, c->stream));
    } else {
        DevBuf<float4> tmp;
        S2D_HIP(c, tmp.alloc(px));
        const IdleAtExit idle{c->stream}; // (before tmp goes)
        S2D_HIP(c, launch_convert_f16_to_f32(c->d_image0, tmp, px, c->stream));
        S2D_HIP(c, hipMemcpyAsync(dst, tmp, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (to_host) S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

// s2d_step (loss == nullptr) and s2d_step_loss: `iters` iterations queued in pieces of the rings' capacity, their squared
// errors (and loss totals) read back per piece, the status word judged once at the end.
int run_steps(s2d_ctx* c, int iters, uint32_t flags, const s2d_loss_config* loss, double* loss_out, double* mse_out)
{
    static_assert(LossTrace::kCapacity == SqerrTrace::kCapacity, "one piece size for both rings");
    WalkFlags wf;
    if (int rc = parse_walk_flags(c, flags, true, &wf)) return rc;
    if (int rc = use_device(c)) return rc;
    const double norm = mse_norm(c);
    const float w[3] = {loss ? loss->w_mse : 0.0f, loss ? loss->w_l1 : 0.0f, loss ? loss->w_dssim : 0.0f};
    const int call_first_iter = c->iterations;
    std::vector<double> sums;
    bool status_read = false;
    for (int done = 0; done < iters;) {
        const int piece = std::min<int>(iters - done, SqerrTrace::kCapacity);
        const int first_iter = c->iterations;
        for (int k = 0; k < piece; k++) {
            if (loss) { // the loss kernels stand between the two walks (image0 stored every time)
                if (int rc = queue_forward(c)) return rc;
                if (int rc = queue_loss_backward(c, loss, wf.need_opacity_grad, wf.density)) return rc;
            } else if (wf.density) { // the separate passes: only s2d_backward's kernel gathers the statistics (image0 stored every time)
                if (int rc = queue_forward(c)) return rc;
                if (int rc = queue_backward(c, wf.need_opacity_grad, nullptr, true)) return rc;
            } else if (int rc = queue_forward_backward(c, wf.need_opacity_grad, done + k + 1 == iters)) {
                return rc; // (image0 is stored by the last iteration of the call only: nothing else could observe the others)
            }
            if (int rc = queue_adam(c, flags)) return rc;
        }
        // The usual call (a frame, or a batch of frames, of the host loop) ends with a piece that fits the pinned buffer:
        // trace and status word in ONE round trip.  Any other piece is read by itself, if there is something to read.
        const bool with_status = done + piece == iters && piece <= SqerrTrace::kPinned;
        double* const mse_dst = !mse_out ? nullptr : with_status ? c->trace.pinned() : mse_out + done;
        if (loss_out) {
            sums.resize((size_t)3 * piece);
            S2D_HIP(c, c->loss.read(first_iter, piece, sums.data()));
        }
        if (mse_dst) S2D_HIP(c, c->trace.read(first_iter, piece, mse_dst));
        if (with_status)
            if (int rc = queue_status_read(c)) return rc;
        if (with_status || loss_out || mse_out) S2D_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; loss_out && k < piece; k++) loss_out[done + k] = loss_terms_of(c, &sums[(size_t)3 * k], w).total;
        for (int k = 0; mse_out && k < piece; k++) mse_out[done + k] = mse_dst[k] / norm; // main.cpp:805
        status_read = with_status;
        done += piece;
    }
    const int rc = status_read ? judge_status(c) : check_status(c);
    if (rc == S2D_E_NONFINITE) {
        // The reference abort()s right after the Adam step of that iteration (main.cpp:752-785): its trace ends with
        // that iteration's line.  The kernels of the later iterations queued here did nothing; their entries are NaN.
        const int last_valid = c->h_status->first_nonfinite_iter - call_first_iter;
        for (int k = std::max(last_valid + 1, 0); k < iters; k++) {
            if (loss_out) loss_out[k] = std::nan("");
            if (mse_out) mse_out[k] = std::nan("");
        }
    }
    return rc;
}

// ---- importance-sampled placement (s2d_seed.h) -----------------------------------------------------------------------
// Everything s2d_importance / s2d_seed_splats / s2d_reseed refuse for the configuration or the context, before any device
// work (S2D_E_INVALID), then what they refuse for the order of calls (S2D_E_STATE).
int seed_refused(s2d_ctx* c, const s2d_seed_config* cfg)
{
    if (!cfg || cfg->struct_size != sizeof(s2d_seed_config)) return fail(c, S2D_E_INVALID, "s2d_seed_config: NULL or wrong struct_size");
    if (cfg->source > S2D_SEED_CALLER) return fail(c, S2D_E_INVALID, "s2d_seed_config: unknown source %u", cfg->source);
    if (cfg->flags & ~S2D_SEED_SQUARED) return fail(c, S2D_E_INVALID, "s2d_seed_config: unknown flags 0x%x", cfg->flags);
    if (cfg->floor > kSeedQMax) return fail(c, S2D_E_INVALID, "s2d_seed_config: floor %u > 4095", cfg->floor);
    if (!(cfg->scale >= 0.0f) || std::isinf(cfg->scale)) return fail(c, S2D_E_INVALID, "s2d_seed_config: scale must be finite and >= 0 (0: sqrt(W H / n))");
    if (!(cfg->opacity >= 0.0f && cfg->opacity <= 1.0f)) return fail(c, S2D_E_INVALID, "s2d_seed_config: opacity must be 0 (meaning 1) or in (0, 1]");
    if ((cfg->source == S2D_SEED_CALLER) != (cfg->importance_device != nullptr))
        return fail(c, S2D_E_INVALID, "s2d_seed_config: importance_device goes with S2D_SEED_CALLER, and only with it");
    if (c->g.row_begin != 0 || c->g.row_end != c->g.H)
        return fail(c, S2D_E_INVALID, "the importance map covers the whole image: this context owns a row slab");
    if (c->state.held()) return fail(c, S2D_E_INVALID, "placement needs every splat: this context holds a subset (s2d_halo_commit)");
    return S2D_OK;
}

int seed_state_refused(s2d_ctx* c, const s2d_seed_config* cfg)
{
    if (!c->have_target) return fail(c, S2D_E_STATE, "no target image set (s2d_set_target)");
    if (cfg->source == S2D_SEED_ERROR && !c->have_forward)
        return fail(c, S2D_E_STATE, "S2D_SEED_ERROR needs s2d_forward on the current parameters");
    return S2D_OK;
}

// The map of the current images (queued) and its total (waits).
int seed_map(s2d_ctx* c, const s2d_seed_config* cfg, SeedMap* map, uint64_t* total)
{
    S2D_HIP(c, c->seed.ensure(slab_pixels(c), map));
    SeedMapArgs a;
    a.source = (SeedSource)cfg->source; a.image0 = c->d_image0; a.image_ref = c->d_ref; a.caller = cfg->importance_device;
    a.half_images = c->half_images; a.W = c->g.W; a.H = c->g.H; a.squared = (cfg->flags & S2D_SEED_SQUARED) != 0; a.floor_q = cfg->floor;
    a.map = *map;
    S2D_HIP(c, launch_seed_map(a, c->stream));
    S2D_HIP(c, hipMemcpyAsync(total, map->share_prefix + (map->shares - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

// The rows `ids` (distinct, in range; null: 0 .. count - 1) drawn from the map of the current images and written; what
// follows a write of some rows (the table above invalidate()).  *placed: count, or 0 for a map whose total is 0.
int seed_rows(s2d_ctx* c, const s2d_seed_config* cfg, const int32_t* ids, int count, int32_t* placed)
{
    *placed = 0;
    SeedMap map;
    uint64_t total = 0;
    if (int rc = seed_map(c, cfg, &map, &total)) return rc;
    if (total == 0 || count == 0) return S2D_OK;
    DevBuf<int32_t> d_ids;
    if (ids) S2D_HIP(c, d_ids.alloc((size_t)count));
    const IdleAtExit idle{c->stream}; // (before d_ids goes, and while `ids` is read)
    if (ids) S2D_HIP(c, hipMemcpyAsync(d_ids, ids, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    SeedPlaceArgs p;
    p.map = map; p.total = total; p.ids = ids ? (const int32_t*)d_ids : nullptr; p.count = count; p.seed = cfg->seed;
    p.image_ref = c->d_ref; p.half_images = c->half_images; p.W = c->g.W; p.H = c->g.H;
    p.scale = seed_scale(cfg->scale, c->g.W, c->g.H, c->n); p.opacity = seed_opacity(cfg->opacity);
    p.splats = now.splats; p.adams = now.adams;
    S2D_HIP(c, launch_seed_place(p, c->stream));
    S2D_HIP(c, c->state.written(false));
    invalidate(c, Stale::Projection); // (as s2d_rows_scatter: the containment check asks for new lists where a row left its rectangle)
    *placed = count;
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_abi_version(void) { return S2D_ABI_VERSION; }

int s2d_create(const s2d_config* cfg, s2d_ctx** out)
{
    if (!cfg || !out || cfg->struct_size != sizeof(s2d_config)) return S2D_E_INVALID;
    *out = nullptr;
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->n_splats < 0 || cfg->width > 65536 || cfg->height > 65536)
        return S2D_E_INVALID;
    int rb = cfg->row_begin, re = cfg->row_end;
    if (rb == 0 && re == 0) re = cfg->height;
    if (rb < 0 || re > cfg->height || rb >= re || (rb % kTile) != 0) return S2D_E_INVALID;
    if ((cfg->flags & (S2D_CFG_EXACT_EXP | S2D_CFG_REFERENCE_ORDER)) && (cfg->flags & (S2D_CFG_COUNT_PAIRS | S2D_CFG_FP16_IMAGES)))
        return S2D_E_INVALID;

    s2d_ctx* c = new (std::nothrow) s2d_ctx();
    if (!c) return S2D_E_NOMEM;
    *out = c; // handed out even on failure so that s2d_last_error works; caller destroys it
    c->cfg = *cfg;
    c->n = cfg->n_splats;
    c->device = cfg->device;
    c->lr = cfg->training_rate > 0.0f ? cfg->training_rate : 0.05f; // main.cpp:715

    Geometry& g = c->g;
    g.W = cfg->width; g.H = cfg->height;
    g.row_begin = rb; g.row_end = re;
    g.tiles_x = (g.W + kTile - 1) / kTile;
    g.trow0 = rb / kTile;
    g.tiles_y = (re + kTile - 1) / kTile - g.trow0;
    g.num_tiles = g.tiles_x * g.tiles_y;

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(c, S2D_E_HIP, "no HIP device available (%s): this library has no CPU fallback", hipGetErrorString(e));
    if (c->device < 0 || c->device >= ndev) return fail(c, S2D_E_INVALID, "device %d out of range (%d devices)", c->device, ndev);
    S2D_HIP(c, hipSetDevice(c->device));
    if (cfg->stream) {
        c->stream = (hipStream_t)cfg->stream;
    } else {
        S2D_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }

    const size_t n = std::max<size_t>((size_t)c->n, 1);           // >= 1 so that n == 0 still has buffers
    const size_t px = (size_t)g.W * (size_t)(g.row_end - g.row_begin); // pixels of the slab: all this context stores
    S2D_HIP(c, c->state.create(c->n, c->stream));
    S2D_HIP(c, c->d_grads_own.alloc(n * 9));
    c->d_grads = c->d_grads_own;
    S2D_HIP(c, c->d_proj.alloc(n));
    S2D_HIP(c, c->d_rects.alloc(n));
    S2D_HIP(c, c->d_counts.alloc(n));
    S2D_HIP(c, c->d_offsets.alloc(n));
    S2D_HIP(c, c->d_scan_temp.alloc(scan_temp_words((int64_t)n)));
    S2D_HIP(c, c->lists.create(g, n, (cfg->flags & S2D_CFG_GENERIC_BINNING) != 0));
    c->ranges.create(g, c->stream);
    const bool ref_order = (cfg->flags & S2D_CFG_REFERENCE_ORDER) != 0; // (alone decides the result: deterministic mode is off then)
    S2D_HIP(c, c->scratch.create(ref_order ? PairScratch::Mode::ReferenceOrder : (cfg->flags & S2D_CFG_DETERMINISTIC) ? PairScratch::Mode::Deterministic
                                           : PairScratch::Mode::Atomic, g, n, c->stream));
    c->half_images = (cfg->flags & S2D_CFG_FP16_IMAGES) != 0;
    c->pixel_bytes = c->half_images ? 8 : sizeof(float4);
    S2D_HIP(c, c->d_image0.alloc(px * c->pixel_bytes));
    S2D_HIP(c, c->d_ref.alloc(px * c->pixel_bytes));
    S2D_HIP(c, c->d_status.alloc(1));
    S2D_HIP(c, c->trace.create(g.num_tiles, c->n, c->d_status, c->stream));
    c->density.create(c->n, c->stream);
    S2D_HIP(c, c->d_counters.alloc(1));
    S2D_HIP(c, c->reuse.create(cfg->rebin_interval, cfg->rebin_margin, c->stream));
    S2D_HIP(c, c->h_status.alloc(1, hipHostMallocDefault));

    S2D_HIP(c, hipMemsetAsync(c->d_grads_own, 0, n * 9 * sizeof(float), c->stream));
    S2D_HIP(c, hipMemsetAsync(c->d_image0, 0, px * c->pixel_bytes, c->stream));
    S2D_HIP(c, hipMemsetAsync(c->d_ref, 0, px * c->pixel_bytes, c->stream));
    S2D_HIP(c, hipMemsetAsync(c->d_counters, 0, sizeof(PairCounters), c->stream));
    *c->h_status = kFreshStatus;
    S2D_HIP(c, hipMemcpyAsync(c->d_status, c->h_status, sizeof(DeviceStatus), hipMemcpyHostToDevice, c->stream));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    // ~16 tiles per splat at init() scales; grown on demand
    int rc = ensure_pair_capacity(c, std::max<uint64_t>((uint64_t)n * 20, 1 << 16));
    if (rc != S2D_OK) return rc;
    return S2D_OK;
}

void s2d_destroy(s2d_ctx* c)
{
    if (!c) return;
    // the buffers, pinned mirrors and events go with their members: on the context's device, behind everything queued on
    // the stream, and before a stream of the context's own (also when the device cannot be selected: freeing needs none)
    if (hipSetDevice(c->device) == hipSuccess && c->stream) (void)hipStreamSynchronize(c->stream);
    const hipStream_t own = c->own_stream ? c->stream : nullptr;
    delete c;
    if (own) (void)hipStreamDestroy(own);
}

const char* s2d_last_error(const s2d_ctx* c) { return c ? c->err : "null context"; }

int s2d_set_target(s2d_ctx* c, const float* rgba32f)
{
    if (!c || !rgba32f) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (int rc = upload_target(c, rgba32f)) return rc;
    c->have_target = true;
    invalidate(c, Stale::Frames);
    return S2D_OK;
}

int s2d_set_target_synthetic(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, launch_synthetic_target(c->d_ref, c->half_images, c->g.W, c->g.H, c->g.row_begin, c->g.row_end, c->stream));
    c->have_target = true;
    invalidate(c, Stale::Frames);
    return S2D_OK;
}

int s2d_init_splats(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, c->trace.settle()); // (the iteration count is about to restart)
    const SplatState::Arrays all = c->state.discard_all(); // every record is new
    S2D_HIP(c, launch_init_splats(all.splats, all.adams, c->n, c->g.W, c->g.H, c->stream));
    if (int rc = splats_replaced(c)) return rc;
    if (c->n > 0) S2D_HIP(c, hipMemsetAsync(c->d_grads, 0, (size_t)c->n * 9 * sizeof(float), c->stream));
    S2D_HIP(c, c->density.reset()); // (statistics of splats that no longer exist)
    c->beta1t = c->good_beta1t = 1.0f; // main.cpp:283-284
    c->beta2t = c->good_beta2t = 1.0f;
    c->iterations = c->good_iterations = 0; // main.cpp:281
    return S2D_OK;
}

int s2d_set_splats(s2d_ctx* c, const s2d_splat* splats)
{
    if (!c || (!splats && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    SplatState::Arrays now; // (with the moments of the held splats: they must not be lost with the compact copy)
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, hipMemcpyAsync(now.splats, splats, (size_t)c->n * sizeof(s2d_splat), hipMemcpyHostToDevice, c->stream));
    if (int rc = splats_replaced(c)) return rc;
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

int s2d_get_splats(s2d_ctx* c, s2d_splat* splats)
{
    if (!c || (!splats && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, hipMemcpyAsync(splats, now.splats, (size_t)c->n * sizeof(s2d_splat), hipMemcpyDeviceToHost, c->stream));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

int s2d_set_adam(s2d_ctx* c, const s2d_splat_adam* adams, float beta1t, float beta2t, int32_t iterations)
{
    if (!c || (!adams && c->n) || iterations < 0) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, c->trace.settle()); // (the iteration count is about to change)
    SplatState::Arrays now; // (with the parameters of the held splats: they must not be lost with the compact copy)
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, hipMemcpyAsync(now.adams, adams, (size_t)c->n * sizeof(s2d_splat_adam), hipMemcpyHostToDevice, c->stream));
    S2D_HIP(c, c->state.written(true));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    c->beta1t = c->good_beta1t = beta1t;
    c->beta2t = c->good_beta2t = beta2t;
    c->iterations = c->good_iterations = iterations;
    return S2D_OK;
}

int s2d_get_adam(s2d_ctx* c, s2d_splat_adam* adams, float* beta1t, float* beta2t, int32_t* iterations)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (adams) {
        SplatState::Arrays now;
        S2D_HIP(c, c->state.current(&now));
        S2D_HIP(c, hipMemcpyAsync(adams, now.adams, (size_t)c->n * sizeof(s2d_splat_adam), hipMemcpyDeviceToHost, c->stream));
        S2D_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (beta1t) *beta1t = c->beta1t;
    if (beta2t) *beta2t = c->beta2t;
    if (iterations) *iterations = c->iterations;
    return S2D_OK;
}

int s2d_forward(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    return queue_forward(c);
}

int s2d_get_image_rows(s2d_ctx* c, float* rgba32f_rows)
{
    if (!c || !rgba32f_rows) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    return download_image0(c, rgba32f_rows, true);
}

int s2d_get_image(s2d_ctx* c, float* rgba32f)
{
    if (!c || !rgba32f) return S2D_E_INVALID;
    // a full-size image goes back (main.cpp:794 uploads all of image0): this context's rows, zeros elsewhere
    const size_t row_floats = (size_t)c->g.W * 4;
    std::memset(rgba32f, 0, (size_t)c->g.row_begin * row_floats * sizeof(float));
    std::memset(rgba32f + (size_t)c->g.row_end * row_floats, 0, (size_t)(c->g.H - c->g.row_end) * row_floats * sizeof(float));
    return s2d_get_image_rows(c, rgba32f + (size_t)c->g.row_begin * row_floats);
}

int s2d_forward_backward(s2d_ctx* c, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    if (flags & S2D_BWD_DENSITY_STATS)
        return fail(c, S2D_E_INVALID, "the fused launch has no density-statistics variant: s2d_forward, then s2d_backward with the flag");
    if (int rc = use_device(c)) return rc;
    return queue_forward_backward(c, !(flags & S2D_BWD_SKIP_OPACITY_GRAD), !(flags & S2D_FB_SKIP_IMAGE));
}

int s2d_backward(s2d_ctx* c, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    WalkFlags wf;
    if (int rc = parse_walk_flags(c, flags, false, &wf)) return rc;
    if (int rc = use_device(c)) return rc;
    return queue_backward(c, wf.need_opacity_grad, nullptr, wf.density);
}

int s2d_backward_image_grads(s2d_ctx* c, const float* dimage_rows_device, uint32_t flags)
{
    if (!c || !dimage_rows_device) return S2D_E_INVALID;
    if ((uintptr_t)dimage_rows_device & 15u) return fail(c, S2D_E_INVALID, "the image gradient must be 16-byte aligned");
    if (c->cfg.flags & S2D_CFG_COUNT_PAIRS)
        return fail(c, S2D_E_INVALID, "pair counting (S2D_CFG_COUNT_PAIRS) has no backward pass from a caller's image gradient");
    WalkFlags wf;
    if (int rc = parse_walk_flags(c, flags, false, &wf)) return rc;
    if (int rc = use_device(c)) return rc;
    return queue_backward(c, wf.need_opacity_grad, reinterpret_cast<const float4*>(dimage_rows_device), wf.density);
}

int s2d_set_splats_device(s2d_ctx* c, const float* splats_device)
{
    if (!c || (!splats_device && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    SplatState::Arrays now; // (with the moments of the held splats: they must not be lost with the compact copy)
    S2D_HIP(c, c->state.current(&now));
    if (c->n > 0)
        S2D_HIP(c, hipMemcpyAsync(now.splats, splats_device, (size_t)c->n * sizeof(s2d_splat), hipMemcpyDeviceToDevice, c->stream));
    S2D_HIP(c, c->state.written(true));
    invalidate(c, Stale::Projection); // (not Lists: see the table above invalidate())
    return S2D_OK;
}

int s2d_get_image_rows_device(s2d_ctx* c, float* rgba32f_rows_device)
{
    if (!c || !rgba32f_rows_device) return S2D_E_INVALID;
    if ((uintptr_t)rgba32f_rows_device & 15u) return fail(c, S2D_E_INVALID, "the image buffer must be 16-byte aligned");
    if (int rc = use_device(c)) return rc;
    return download_image0(c, rgba32f_rows_device, false);
}

int s2d_get_grads(s2d_ctx* c, s2d_splat* dsplats)
{
    if (!c || (!dsplats && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, hipMemcpyAsync(dsplats, c->d_grads, (size_t)c->n * sizeof(s2d_splat), hipMemcpyDeviceToHost, c->stream));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

int s2d_density_get_device(s2d_ctx* c, float* out_device, int32_t* passes)
{
    if (!c || (!out_device && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    const size_t bytes = (size_t)c->n * sizeof(s2d_density);
    if (bytes && c->density.data()) S2D_HIP(c, hipMemcpyAsync(out_device, c->density.data(), bytes, hipMemcpyDeviceToDevice, c->stream));
    else if (bytes) S2D_HIP(c, hipMemsetAsync(out_device, 0, bytes, c->stream));
    if (passes) *passes = c->density.passes();
    return S2D_OK;
}

int s2d_density_get(s2d_ctx* c, s2d_density* host, int32_t* passes)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    const size_t bytes = (size_t)c->n * sizeof(s2d_density);
    if (host && bytes && c->density.data()) {
        S2D_HIP(c, hipMemcpyAsync(host, c->density.data(), bytes, hipMemcpyDeviceToHost, c->stream));
        S2D_HIP(c, hipStreamSynchronize(c->stream));
    } else if (host && bytes) {
        std::memset(host, 0, bytes);
    }
    if (passes) *passes = c->density.passes();
    return S2D_OK;
}

int s2d_density_reset(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, c->density.reset());
    return S2D_OK;
}

int s2d_relocate(s2d_ctx* c, const s2d_relocate_config* cfg, int32_t* moved)
{
    if (!c || !cfg || cfg->struct_size != sizeof(s2d_relocate_config)) return S2D_E_INVALID;
    if (moved) *moved = 0;
    const float shrink = cfg->shrink == 0.0f ? 1.6f : cfg->shrink;
    if (cfg->max_moves < 0 || !(shrink > 0.0f) || std::isinf(shrink) || std::isnan(cfg->min_weight))
        return fail(c, S2D_E_INVALID, "s2d_relocate: max_moves >= 0, a finite shrink > 0 (0: 1.6) and a min_weight that is a number");
    if (c->g.row_begin != 0 || c->g.row_end != c->g.H)
        return fail(c, S2D_E_INVALID, "s2d_relocate needs the statistics of the whole image: this context owns a row slab");
    if (c->state.held()) return fail(c, S2D_E_INVALID, "s2d_relocate: this context holds a subset of the splats (s2d_halo_commit)");
    if (c->scratch.reference_order()) return fail(c, S2D_E_INVALID, "s2d_relocate is not available with S2D_CFG_REFERENCE_ORDER");
    const int passes = c->density.passes();
    if (passes == 0) return fail(c, S2D_E_STATE, "s2d_relocate needs a pass with S2D_BWD_DENSITY_STATS since the last reset");
    if (int rc = use_device(c)) return rc;
    const size_t n = (size_t)c->n;
    std::vector<float> stats(n * 3), splats(n * 9), adams(n * 18);
    std::vector<int32_t> ids(2 * std::min<size_t>((size_t)cfg->max_moves, n));
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    if (n > 0) {
        S2D_HIP(c, hipMemcpyAsync(stats.data(), c->density.data(), n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        S2D_HIP(c, hipMemcpyAsync(splats.data(), now.splats, n * 9 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        S2D_HIP(c, hipMemcpyAsync(adams.data(), now.adams, n * 18 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    const int moves = density_plan(c->n, stats.data(), passes, cfg->max_moves, cfg->min_weight, shrink, c->g.W, c->g.H, splats.data(),
                                   adams.data(), ids.data());
    if (moves > 0) { // the changed rows, through the row calls' scatter
        const size_t rows = 2 * (size_t)moves;
        std::vector<float> srows(rows * 9), arows(rows * 18);
        for (size_t r = 0; r < rows; r++) {
            std::memcpy(&srows[r * 9], &splats[(size_t)ids[r] * 9], 9 * sizeof(float));
            std::memcpy(&arows[r * 18], &adams[(size_t)ids[r] * 18], 18 * sizeof(float));
        }
        DevBuf<int32_t> d_ids;
        DevBuf<float> d_srows, d_arows;
        S2D_HIP(c, d_ids.alloc(rows));
        S2D_HIP(c, d_srows.alloc(rows * 9));
        S2D_HIP(c, d_arows.alloc(rows * 18));
        const IdleAtExit idle{c->stream}; // (before the three go)
        S2D_HIP(c, hipMemcpyAsync(d_ids, ids.data(), rows * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        S2D_HIP(c, hipMemcpyAsync(d_srows, srows.data(), rows * 9 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        S2D_HIP(c, hipMemcpyAsync(d_arows, arows.data(), rows * 18 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        S2D_HIP(c, launch_rows_scatter(now.splats, 9, d_ids, (int)rows, c->n, d_srows, c->stream));
        S2D_HIP(c, launch_rows_scatter(now.adams, 18, d_ids, (int)rows, c->n, d_arows, c->stream));
        S2D_HIP(c, c->state.written(false));
        invalidate(c, Stale::Projection); // (as s2d_rows_scatter: the containment check asks for new lists where a row left its rectangle)
        S2D_HIP(c, hipStreamSynchronize(c->stream)); // (the host copies are read by the stream until here)
    }
    S2D_HIP(c, c->density.reset());
    if (moved) *moved = moves;
    return S2D_OK;
}

int s2d_importance(s2d_ctx* c, const s2d_seed_config* cfg, uint32_t* q_host, uint64_t* total)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = seed_refused(c, cfg)) return rc;
    if (int rc = seed_state_refused(c, cfg)) return rc;
    if (int rc = use_device(c)) return rc;
    SeedMap map;
    uint64_t sum = 0;
    if (int rc = seed_map(c, cfg, &map, &sum)) return rc;
    if (q_host) {
        S2D_HIP(c, hipMemcpyAsync(q_host, map.q, map.pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        S2D_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (total) *total = sum;
    return S2D_OK;
}

int s2d_seed_splats(s2d_ctx* c, const s2d_seed_config* cfg, const int32_t* ids_host, int32_t count, int32_t* placed)
{
    if (!c) return S2D_E_INVALID;
    if (placed) *placed = 0;
    if (int rc = seed_refused(c, cfg)) return rc;
    if (count < 0 || count > c->n) return fail(c, S2D_E_INVALID, "s2d_seed_splats: count %d outside 0 .. n_splats", count);
    if (ids_host) {
        std::vector<bool> seen((size_t)c->n, false);
        for (int j = 0; j < count; j++) {
            const int32_t i = ids_host[j];
            if (i < 0 || i >= c->n || seen[(size_t)i]) return fail(c, S2D_E_INVALID, "s2d_seed_splats: ids[%d] = %d is out of range or repeated", j, i);
            seen[(size_t)i] = true;
        }
    }
    if (int rc = seed_state_refused(c, cfg)) return rc;
    if (int rc = use_device(c)) return rc;
    int32_t done = 0;
    if (int rc = seed_rows(c, cfg, ids_host, count, &done)) return rc;
    if (placed) *placed = done;
    return S2D_OK;
}

int s2d_reseed(s2d_ctx* c, const s2d_seed_config* cfg, int32_t max_moves, float min_weight, int32_t* moved)
{
    if (!c) return S2D_E_INVALID;
    if (moved) *moved = 0;
    if (int rc = seed_refused(c, cfg)) return rc;
    if (max_moves < 0 || std::isnan(min_weight)) return fail(c, S2D_E_INVALID, "s2d_reseed: max_moves >= 0 and a min_weight that is a number");
    if (c->scratch.reference_order()) return fail(c, S2D_E_INVALID, "s2d_reseed is not available with S2D_CFG_REFERENCE_ORDER");
    if (int rc = seed_state_refused(c, cfg)) return rc;
    const int passes = c->density.passes();
    if (passes == 0) return fail(c, S2D_E_STATE, "s2d_reseed needs a pass with S2D_BWD_DENSITY_STATS since the last reset");
    if (int rc = use_device(c)) return rc;
    const size_t n = (size_t)c->n;
    std::vector<float> stats(n * 3);
    std::vector<int32_t> ids(std::min<size_t>((size_t)max_moves, n));
    if (n > 0) S2D_HIP(c, hipMemcpyAsync(stats.data(), c->density.data(), n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    const int starved = density_starved(c->n, stats.data(), passes, max_moves, min_weight, ids.data());
    int32_t done = 0;
    if (starved > 0)
        if (int rc = seed_rows(c, cfg, ids.data(), starved, &done)) return rc;
    S2D_HIP(c, c->density.reset());
    if (moved) *moved = done;
    return S2D_OK;
}

int s2d_loss_image_grads_device(s2d_ctx* c, const s2d_loss_config* cfg, float* dimage_rows_device)
{
    if (!c || !dimage_rows_device) return S2D_E_INVALID;
    if (int rc = loss_refused(c, cfg)) return rc;
    if ((uintptr_t)dimage_rows_device & 15u) return fail(c, S2D_E_INVALID, "the image gradient must be 16-byte aligned");
    if (int rc = use_device(c)) return rc;
    return queue_loss(c, cfg, reinterpret_cast<float4*>(dimage_rows_device), LossTrace::kEvalSlot, nullptr);
}

int s2d_loss_backward(s2d_ctx* c, const s2d_loss_config* cfg, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = loss_refused(c, cfg)) return rc;
    WalkFlags wf;
    if (int rc = parse_walk_flags(c, flags, false, &wf)) return rc;
    if (int rc = use_device(c)) return rc;
    return queue_loss_backward(c, cfg, wf.need_opacity_grad, wf.density);
}

int s2d_loss_get(s2d_ctx* c, s2d_loss_terms* out)
{
    if (!c || !out) return S2D_E_INVALID;
    if (c->loss.last_slot() < 0) return fail(c, S2D_E_STATE, "no loss pass has run yet");
    if (int rc = use_device(c)) return rc;
    double sums[3];
    S2D_HIP(c, hipMemcpyAsync(sums, c->loss.slot(c->loss.last_slot()), sizeof(sums), hipMemcpyDeviceToHost, c->stream));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    *out = loss_terms_of(c, sums, c->loss.last_weights());
    return S2D_OK;
}

int s2d_step_loss(s2d_ctx* c, int32_t iters, uint32_t flags, const s2d_loss_config* cfg, double* loss_out, double* mse_out)
{
    if (!c || iters < 0) return S2D_E_INVALID;
    if (int rc = loss_refused(c, cfg)) return rc;
    return run_steps(c, iters, flags, cfg, loss_out, mse_out);
}

int s2d_adam_step(s2d_ctx* c, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (int rc = queue_adam(c, flags)) return rc;
    return S2D_OK;
}

int s2d_step(s2d_ctx* c, int32_t iters, uint32_t flags, double* mse_out)
{
    if (!c || iters < 0) return S2D_E_INVALID;
    return run_steps(c, iters, flags, nullptr, nullptr, mse_out);
}

int s2d_get_mse(s2d_ctx* c, double* mse)
{
    if (!c || !mse) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (c->trace.last_iteration() < 0) return fail(c, S2D_E_STATE, "no backward pass has run yet");
    double v = 0.0;
    S2D_HIP(c, c->trace.read(c->trace.last_iteration(), 1, &v));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    *mse = v / mse_norm(c);
    return S2D_OK;
}

int s2d_bind_grads_device(s2d_ctx* c, void* grads_device)
{
    if (!c) return S2D_E_INVALID;
    if ((uintptr_t)grads_device & 15u) return fail(c, S2D_E_INVALID, "the gradient buffer must be 16-byte aligned");
    c->d_grads = grads_device ? (float*)grads_device : c->d_grads_own;
    return S2D_OK;
}

void* s2d_grads_device_ptr(s2d_ctx* c) { return c ? (void*)c->d_grads : nullptr; }

void* s2d_stream(s2d_ctx* c) { return c ? (void*)c->stream : nullptr; }

// ---- slab ownership (s2d_halo.hip): all pointers below are device pointers of the caller ----

int s2d_halo_masks(s2d_ctx* c, int32_t world, const int32_t* row_bounds, float margin_rows, uint32_t* masks_device)
{
    if (!c || !row_bounds || !masks_device || world < 1 || world > 32 || !(margin_rows >= 0.0f)) return S2D_E_INVALID;
    for (int q = 0; q < world; q++)
        if (row_bounds[q] > row_bounds[q + 1]) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, launch_halo_masks(now.splats, c->state.held(), c->n, world, row_bounds, margin_rows, masks_device, c->stream));
    return S2D_OK;
}

int s2d_halo_commit(s2d_ctx* c, const uint32_t* masks_device, int32_t rank, int32_t added)
{
    if (!c || rank < 0 || rank > 31) return S2D_E_INVALID;
    if (masks_device && c->scratch.reference_order())
        return fail(c, S2D_E_INVALID, "reference order (S2D_CFG_REFERENCE_ORDER) has no slab ownership: the chains run over all splats");
    if (int rc = use_device(c)) return rc;
    const bool had = c->state.held() != nullptr;
    S2D_HIP(c, c->state.commit(masks_device, rank, c->d_scan_temp));
    // the lists hold the held splats only.  Splats arrived, or this is the first held set: project the held ones and
    // rebuild the lists before the next forward; so on the return to holding everything
    if (masks_device ? (added || !had) : had) invalidate(c, Stale::Lists);
    return S2D_OK;
}

// The array of a row call and its row width, on the context's device: the gradients, or the state's arrays with
// everything queued so far in them.
static int rows_base(s2d_ctx* c, int32_t what, float** base, int* w)
{
    if (what != S2D_ROWS_GRADS && what != S2D_ROWS_SPLATS && what != S2D_ROWS_ADAM) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    *base = c->d_grads;
    *w = what == S2D_ROWS_ADAM ? 18 : 9;
    if (what == S2D_ROWS_GRADS) return S2D_OK;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    *base = what == S2D_ROWS_SPLATS ? now.splats : now.adams;
    return S2D_OK;
}

int s2d_rows_gather(s2d_ctx* c, int32_t what, const int32_t* ids_device, int32_t count, float* out_device)
{
    if (!c || count < 0 || (count > 0 && (!ids_device || !out_device))) return S2D_E_INVALID;
    float* base;
    int w;
    if (int rc = rows_base(c, what, &base, &w)) return rc;
    S2D_HIP(c, launch_rows_gather(base, w, ids_device, count, c->n, out_device, c->stream));
    return S2D_OK;
}

int s2d_rows_scatter(s2d_ctx* c, int32_t what, const int32_t* ids_device, int32_t count, const float* in_device)
{
    if (!c || count < 0 || (count > 0 && (!ids_device || !in_device))) return S2D_E_INVALID;
    float* base;
    int w;
    if (int rc = rows_base(c, what, &base, &w)) return rc;
    S2D_HIP(c, launch_rows_scatter(base, w, ids_device, count, c->n, in_device, c->stream));
    if (what != S2D_ROWS_GRADS) S2D_HIP(c, c->state.written(false));
    if (what == S2D_ROWS_SPLATS) invalidate(c, Stale::Projection); // parameters changed behind the projection
    return S2D_OK;
}

int s2d_grads_combine(s2d_ctx* c, const int32_t* rows_device, int32_t n_rows, const int32_t* src_device, int32_t world,
                      const float* recv_device)
{
    if (!c || n_rows < 0 || world < 1 || world > 32 || (n_rows > 0 && (!rows_device || !src_device))) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, launch_grads_combine(c->d_grads, rows_device, n_rows, src_device, world, recv_device, c->n, c->stream));
    return S2D_OK;
}

int s2d_get_sqerr_trace(s2d_ctx* c, int32_t first_iteration, int32_t count, double* out)
{
    if (!c || !out || count < 0 || first_iteration < 0 || count > SqerrTrace::kCapacity) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, c->trace.read(first_iteration, count, out));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

int s2d_synchronize(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    return check_status(c);
}

int s2d_get_stats(s2d_ctx* c, s2d_stats* out)
{
    // the struct as its first version (ABI 2) ends with bwd_quadrant_execs: a caller must have at least that
    if (!c || !out || out->struct_size < (uint32_t)(offsetof(s2d_stats, bwd_quadrant_execs) + sizeof(uint64_t))) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    PairCounters pc;
    S2D_HIP(c, hipMemcpyAsync(&pc, c->d_counters, sizeof(pc), hipMemcpyDeviceToHost, c->stream));
    if (int rc = queue_status_read(c)) return rc;
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    // filled in a full-size copy, handed back at the caller's size: a caller built against an older, shorter struct is
    // never written past its end
    const uint32_t caller_size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(s2d_stats));
    s2d_stats full;
    s2d_stats* const dst = out;
    out = &full;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = caller_size;
    out->pairs_binned = c->lists.pairs();
    out->pairs_capacity = c->lists.capacity();
    out->rebins = c->lists.builds();
    out->fwd_visited = pc.fwd_visited; out->fwd_active = pc.fwd_active;
    out->bwd_visited = pc.bwd_visited; out->bwd_active = pc.bwd_active;
    out->fwd_staged = pc.fwd_staged; out->bwd_staged = pc.bwd_staged;
    out->fwd_wave_execs = pc.fwd_wave_execs; out->bwd_wave_execs = pc.bwd_wave_execs;
    for (int k = 0; k < 65; k++) out->bwd_lane_hist[k] = pc.bwd_lane_hist[k];
    out->fwd_staged_hit = pc.fwd_staged_hit;
    out->fwd_rows_hit = pc.fwd_rows_hit;
    out->bwd_quadrant_execs = pc.bwd_quadrant_execs;
    out->iterations = c->iterations;
    out->first_nonfinite_iteration = c->h_status->nonfinite ? c->h_status->first_nonfinite_iter : -1;
    std::memcpy(dst, &full, caller_size);
    return S2D_OK;
}

int s2d_get_rebuild_count(const s2d_ctx* c, uint64_t* rebuilds)
{
    if (!c || !rebuilds) return S2D_E_INVALID;
    *rebuilds = c->lists.builds();
    return S2D_OK;
}

int s2d_debug_get_tile_lists(s2d_ctx* c, int32_t* tiles_x, int32_t* tiles_y, uint32_t* offsets,
                             int64_t offsets_capacity, uint32_t* list, int64_t list_capacity)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (!c->lists_valid) return fail(c, S2D_E_STATE, "tile lists not built yet (run s2d_forward)");
    if (tiles_x) *tiles_x = c->g.tiles_x;
    if (tiles_y) *tiles_y = c->g.tiles_y;
    if (offsets) {
        if (offsets_capacity < c->g.num_tiles + 1) return S2D_E_INVALID;
        S2D_HIP(c, hipMemcpyAsync(offsets, c->lists.tile_off(), (size_t)(c->g.num_tiles + 1) * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, c->stream));
    }
    if (list) {
        if (list_capacity < (int64_t)c->lists.pairs()) return S2D_E_INVALID;
        S2D_HIP(c, hipMemcpyAsync(list, c->lists.list(), (size_t)c->lists.pairs() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

// ---- test hooks -----------------------------------------------------------------------------------
// (no context: S2D_HIP(nullptr, ...) reports S2D_E_HIP without a message; the owners free on every way out)
int s2d_test_sincos(int32_t device, const float* x, int32_t n, float* sin_out, float* cos_out)
{
    if (!x || !sin_out || !cos_out || n < 0) return S2D_E_INVALID;
    DevBuf<float> dx, ds, dc;
    S2D_HIP(nullptr, hipSetDevice(device));
    S2D_HIP(nullptr, dx.alloc((size_t)n));
    S2D_HIP(nullptr, ds.alloc((size_t)n));
    S2D_HIP(nullptr, dc.alloc((size_t)n));
    S2D_HIP(nullptr, hipMemcpy(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    S2D_HIP(nullptr, launch_test_sincos(dx, n, ds, dc, nullptr));
    S2D_HIP(nullptr, hipDeviceSynchronize());
    S2D_HIP(nullptr, hipMemcpy(sin_out, ds, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    S2D_HIP(nullptr, hipMemcpy(cos_out, dc, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return S2D_OK;
}

int s2d_test_sort_pairs(int32_t device, uint32_t* keys, uint32_t* values, int64_t n, int32_t key_bits)
{
    if (!keys || !values || n < 0 || key_bits < 0 || key_bits > 32) return S2D_E_INVALID;
    DevBuf<uint32_t> k[2], v[2], temp;
    uint32_t *ko = nullptr, *vo = nullptr;
    S2D_HIP(nullptr, hipSetDevice(device));
    for (int i = 0; i < 2; i++) {
        S2D_HIP(nullptr, k[i].alloc((size_t)n));
        S2D_HIP(nullptr, v[i].alloc((size_t)n));
    }
    S2D_HIP(nullptr, temp.alloc(sort_temp_words(n)));
    S2D_HIP(nullptr, hipMemcpy(k[0], keys, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    S2D_HIP(nullptr, hipMemcpy(v[0], values, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    S2D_HIP(nullptr, sort_pairs_u32(k[0], v[0], k[1], v[1], n, key_bits, temp, &ko, &vo, nullptr, nullptr));
    S2D_HIP(nullptr, hipDeviceSynchronize());
    S2D_HIP(nullptr, hipMemcpy(keys, ko, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    S2D_HIP(nullptr, hipMemcpy(values, vo, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return S2D_OK;
}

// The generic builder's last steps (TileLists::finish): the sort whose last pass records where every key's pairs begin
// instead of writing the sorted keys, then the offsets from those.  Keys must be tile ids, < num_keys: the last pass
// indexes tile_first with the whole key.
int s2d_test_sort_tile_offsets(int32_t device, const uint32_t* keys, uint32_t* values, int64_t n, int32_t num_keys,
                               uint32_t* tile_off)
{
    if (!keys || !values || !tile_off || n < 0 || n > 0xFFFFFFFFll || num_keys < 2 || num_keys > (1 << 30)) return S2D_E_INVALID;
    for (int64_t i = 0; i < n; i++)
        if (keys[i] >= (uint32_t)num_keys) return S2D_E_INVALID;
    int key_bits = 0;
    while ((1 << key_bits) < num_keys) key_bits++;
    DevBuf<uint32_t> k[2], v[2], temp, first, off;
    uint32_t *ko = nullptr, *vo = nullptr;
    S2D_HIP(nullptr, hipSetDevice(device));
    for (int i = 0; i < 2; i++) {
        S2D_HIP(nullptr, k[i].alloc((size_t)n));
        S2D_HIP(nullptr, v[i].alloc((size_t)n));
    }
    S2D_HIP(nullptr, temp.alloc(sort_temp_words(n)));
    S2D_HIP(nullptr, first.alloc(((size_t)1 << key_bits) + tile_first_temp_words(num_keys)));
    S2D_HIP(nullptr, off.alloc((size_t)num_keys + 1));
    S2D_HIP(nullptr, hipMemcpy(k[0], keys, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    S2D_HIP(nullptr, hipMemcpy(v[0], values, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    S2D_HIP(nullptr, hipMemsetAsync(first, 0xFF, ((size_t)1 << key_bits) * sizeof(uint32_t), nullptr));
    S2D_HIP(nullptr, sort_pairs_u32(k[0], v[0], k[1], v[1], n, key_bits, temp, &ko, &vo, first, nullptr));
    S2D_HIP(nullptr, launch_tile_offsets_from_first(first, num_keys, (uint32_t)n, first + ((size_t)1 << key_bits), off, nullptr));
    S2D_HIP(nullptr, hipDeviceSynchronize());
    S2D_HIP(nullptr, hipMemcpy(values, vo, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    S2D_HIP(nullptr, hipMemcpy(tile_off, off, ((size_t)num_keys + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return S2D_OK;
}

int s2d_test_exclusive_scan(int32_t device, uint32_t* data, int64_t n, uint64_t* total)
{
    if (!data || n < 0) return S2D_E_INVALID;
    DevBuf<uint32_t> d, temp, tot;
    uint32_t htot = 0;
    S2D_HIP(nullptr, hipSetDevice(device));
    S2D_HIP(nullptr, d.alloc((size_t)n));
    S2D_HIP(nullptr, temp.alloc(scan_temp_words(n)));
    S2D_HIP(nullptr, tot.alloc(1));
    S2D_HIP(nullptr, hipMemcpy(d, data, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    S2D_HIP(nullptr, exclusive_scan_u32(d, d, n, temp, tot, nullptr));
    S2D_HIP(nullptr, hipDeviceSynchronize());
    S2D_HIP(nullptr, hipMemcpy(data, d, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    S2D_HIP(nullptr, hipMemcpy(&htot, tot, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (total) *total = htot;
    return S2D_OK;
}

} // extern "C"
