// s2d_sequence.hip -- the sequencing of one iteration on the context's stream, and the events that make what it derived
// stale (s2d_sequence.h).
//
// One iteration (main.cpp:414-809) of s2d_step is TWO launches on the context's stream:
//   raster_fused (forward walk + backward walk + per-tile squared error of every tile)
//   -> adam (+ the sum of the tile errors, + projection of the updated splats and the containment check for the next
//      iteration)
// s2d_forward / s2d_backward / s2d_adam_step queue the passes one by one (raster_forward, raster_backward, sqerr_finalize).
// When the tile lists have to be (re)built:  project -> TileLists (s2d_lists.h): count scan -> emit -> sort -> tile offsets.
// The host never makes the GPU wait: it reads the 4-byte containment flag after launching the raster kernel
// optimistically, and the 4-byte pair count only when lists are rebuilt.
#include "s2d_ctx.h"

#include <algorithm>
#include <cmath>
#include <vector>

// Room for `need` pairs in the training image's lists and scratch (RasterSurface::ensure_pairs), in the context's words.
int ensure_pair_capacity(s2d_ctx* c, uint64_t need)
{
    if (need >= kMaxPairs) return fail(c, S2D_E_NOMEM, "tile lists need %llu pairs (> 2^32)", (unsigned long long)need);
    PairScratch::Grant refused{};
    const hipError_t e = c->surface.ensure_pairs(need, true, &refused);
    if (refused.refused)
        return fail(c, S2D_E_NOMEM, "the term scratch of S2D_CFG_REFERENCE_ORDER needs %llu bytes for %llu (tile, splat) pairs, "
                    "S2D_REFERENCE_ORDER_MAX_BYTES allows %llu", (unsigned long long)refused.bytes, (unsigned long long)refused.refused,
                    (unsigned long long)c->surface.max_bytes());
    if (e != hipSuccess) return fail(c, S2D_E_HIP, "growing the pair buffers to %llu pairs failed: %s", (unsigned long long)need, hipGetErrorString(e));
    return S2D_OK;
}

namespace {

// (Re)build the per-tile lists from the current parameters.  The projection has already been queued with mode 0.
// first / count: the index range of the splats to list (count < 0: all of them).  A range's lists hold indices RELATIVE to
// its first splat -- every per-splat array is handed over from that splat on -- and so do the scanned offsets.
// *need_ranges (all splats only): their pairs exceed the budget of one set of lists, nothing was built.
int rebuild_lists(s2d_ctx* c, int first = 0, int count = -1, bool* need_ranges = nullptr)
{
    const int n = count < 0 ? c->n : count;
    uint64_t total = 0;
    c->fresh.lists_in_the_making();
    S2D_HIP(c, c->surface.count(first, n, c->d_scan_temp, &total));
    if (need_ranges) *need_ranges = total > c->ranges.budget();
    if (need_ranges && *need_ranges) return S2D_OK;
    if (total >= kMaxPairs)
        return fail(c, S2D_E_NOMEM, "the tile lists of splats %d..%d need more than 2^32 - 65536 (tile, splat) pairs", first, first + n - 1);
    if (int rc = ensure_pair_capacity(c, total)) return rc;
    S2D_HIP(c, c->surface.finish());
    c->fresh.lists_built(count < 0);
    return S2D_OK;
}

// What a raster pass of the context works on: the lists of all splats, or (range >= 0) those of one index range.  A
// range's lists hold indices relative to its first splat, so every per-splat array is handed over from that splat on.
RasterArgs raster_args(const s2d_ctx* c, int range = -1)
{
    const int first = range < 0 ? 0 : c->ranges.first(range), count = range < 0 ? c->n : c->ranges.size(range);
    RasterArgs a;
    c->surface.fill(&a, first, count);
    a.grads = c->d_grads + (size_t)first * 9;
    a.image0 = c->d_image0; a.image_ref = c->d_ref; a.tile_sqerr = c->trace.tile_sqerr();
    a.g = c->g; a.status = c->d_status; a.iteration = c->iterations; a.counters = c->d_counters;
    c->ranges.fill(&a, range);
    a.half_images = c->half_images; a.count = (c->cfg.flags & S2D_CFG_COUNT_PAIRS) != 0; a.exact_exp = (c->cfg.flags & S2D_CFG_EXACT_EXP) != 0;
    a.coverage = coverage(c);
    a.backdrop = c->backdrop.args();
    return a;
}

// What a projection pass works on.  check == nullptr (mode 0): rectangles (inflated by the re-use margin), pair and row
// counts for a list build; otherwise (mode 1): that containment check against those rectangles.
ProjectArgs project_args(const s2d_ctx* c, const float* splats, const ContainmentCheck* check)
{
    ProjectArgs a = c->surface.project_args(splats, c->state.held(), c->n, check ? 0.0f : c->reuse.margin());
    a.check.status = c->d_status;
    if (check) a.mode = 1, a.row_counts = nullptr, a.check = *check;
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
    a.proj = project ? c->surface.proj() : nullptr;
    a.proj_current = c->fresh.projection(); // (every event that replaces parameters clears it)
    a.check = project ? c->reuse.next_check(c->surface.rects(), c->d_status) : c->reuse.idle_check(c->surface.rects(), c->d_status);
    a.sq = c->trace.take_for_adam();
    if (c->has_optim || c->has_frozen) { // the second instantiation: the nine per-field rates of this iteration, the mask
        float group[kOptimGroups];
        optim_rates_at(c->has_optim ? &c->optim : nullptr, c->lr, c->iterations, group);
        a.controls = true;
        for (int k = 0; k < 9; k++) a.rates.r[k] = group[kOptimGroupOf[k]];
        a.frozen = c->has_frozen ? (const uint8_t*)c->d_frozen : nullptr;
    }
    return a;
}

// The pass has a backward walk (deterministic mode: with a fresh stamp for its slots).
void with_backward_walk(s2d_ctx* c, RasterArgs& a, bool need_opacity_grad) { a.need_opacity_grad = need_opacity_grad, c->surface.backward_walk(&a); }

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
    S2D_HIP(c, launch_raster(job.fused ? RasterPass::Fused : RasterPass::Forward, a, c->stream));
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
    if (!c->fresh.target()) return fail(c, S2D_E_STATE, "no target image set (s2d_set_target)");
    const bool scheduled = c->reuse.rebuild_scheduled(c->fresh.lists());
    bool rebuild = scheduled;
    bool stored_image0 = !job.fused || job.write_image; // a fused launch told not to store image0 leaves an older frame there
    if (!scheduled) {
        if (!c->fresh.projection()) { // parameters changed without a fused projection: project + check now
            const ContainmentCheck check = c->reuse.next_check(c->surface.rects(), c->d_status);
            if (int rc = queue_project(c, &check)) return rc;
            S2D_HIP(c, c->reuse.check_queued());
            c->fresh.projected();
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
        if (need_ranges && coverage(c))
            return fail(c, S2D_E_NOMEM, "the coverage channel (S2D_CFG_COVERAGE) is not available for scenes beyond %llu (tile, splat) pairs",
                        (unsigned long long)c->ranges.budget());
        if (need_ranges && c->backdrop.set())
            return fail(c, S2D_E_NOMEM, "a backdrop is not available for scenes beyond %llu (tile, splat) pairs (index-range rendering)",
                        (unsigned long long)c->ranges.budget());
        if (need_ranges && c->surface.reference_order())
            return fail(c, S2D_E_NOMEM, "reference order (S2D_CFG_REFERENCE_ORDER) is not available for scenes beyond %llu (tile, splat) pairs",
                        (unsigned long long)c->ranges.budget());
        c->fresh.projected();
        c->reuse.lists_rebuilt();
        if (need_ranges) {
            // more pairs than one set of lists may hold: render by index ranges (every pass rebuilds: the last range's lists are no lists of the scene)
            S2D_HIP(c, c->ranges.plan(c->surface.counts(), c->n));
            if ((rc = chunked_forward(c)) != S2D_OK) return rc;
            if (job.fused && (rc = chunked_backward(c, job.need_opacity_grad)) != S2D_OK) return rc;
            stored_image0 = true; // the forward pass over the ranges always stores it
        } else if ((rc = launch_job(c, false, job)) != S2D_OK) {
            return rc;
        }
    }
    c->fresh.frame_stored(stored_image0);
    return S2D_OK;
}

} // namespace

int queue_forward(s2d_ctx* c) { return queue_raster(c, RasterJob{}); }

// A backward pass of the current iteration has been queued; `by`: what becomes of its squared error (SqerrTrace::plan,
// or what the pass has done about it already).
int backward_queued(s2d_ctx* c, SqerrBy by)
{
    c->fresh.backward_queued();
    S2D_HIP(c, c->trace.record(c->iterations, by));
    return S2D_OK;
}

// S2D_CFG_REFERENCE_ORDER: terms into their slots, the ordered sums into the gradient buffer, and the squared error as one
// ordered chain straight into the ring slot -- nothing is left to the Adam launch.  (Such a context never renders by
// index ranges, queue_raster refuses the scene, and holds every splat: the state's write-back is a no-op.)
static int queue_backward_reference(s2d_ctx* c, bool need_opacity_grad, const float4* upstream)
{
    RasterArgs a = raster_args(c);
    a.upstream = upstream;
    a.need_opacity_grad = need_opacity_grad;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    const RefOrder ro = c->surface.reference_walk(now.splats, c->n);
    S2D_HIP(c, launch_reference_backward(a, ro, c->stream));
    if (upstream) return backward_queued(c, SqerrBy::NoLoss);
    S2D_HIP(c, launch_reference_sqerr(c->surface.pixel_sqerr(), (size_t)c->g.W * (size_t)(c->g.row_end - c->g.row_begin),
                                      c->trace.job(c->iterations).out, c->d_status, c->iterations, c->stream));
    return backward_queued(c, SqerrBy::PassItself);
}

// What the flags of a backward pass (S2D_BWD_*) or of a step (step: S2D_STEP_*) ask of the backward walk.  The density
// statistics are refused here for a context whose configuration has no such walk (the STATS kernels exist without pair
// counting and the exact exponential; reference order has kernels of its own).
int parse_walk_flags(s2d_ctx* c, uint32_t flags, bool step, WalkFlags* out)
{
    out->need_opacity_grad = step ? (flags & S2D_STEP_OPTIMIZE_OPACITY) != 0 : !(flags & S2D_BWD_SKIP_OPACITY_GRAD);
    out->density = (flags & (step ? S2D_STEP_DENSITY_STATS : S2D_BWD_DENSITY_STATS)) != 0;
    if (out->density && ((c->cfg.flags & (S2D_CFG_COUNT_PAIRS | S2D_CFG_EXACT_EXP | S2D_CFG_COVERAGE)) || c->surface.reference_order()))
        return fail(c, S2D_E_INVALID, "density statistics are not available with S2D_CFG_COUNT_PAIRS, S2D_CFG_EXACT_EXP, "
                    "S2D_CFG_REFERENCE_ORDER or S2D_CFG_COVERAGE");
    return S2D_OK;
}

// upstream != nullptr (s2d_backward_image_grads): the walk starts from the caller's dL/d(image0) instead of
// image0 - imageRef.  The loss is the caller's, so no squared error is formed or queued: the trace ring and a sum still
// waiting for the next Adam launch stay as the last s2d_backward left them (SqerrBy::NoLoss).
// density (S2D_BWD_DENSITY_STATS; parse_walk_flags() has admitted it): the walk also accumulates the density statistics.
int queue_backward(s2d_ctx* c, bool need_opacity_grad, const float4* upstream, bool density)
{
    if (!c->fresh.forward()) return fail(c, S2D_E_STATE, "the backward pass needs s2d_forward on the current parameters");
    if (!upstream && c->weights.set()) return queue_weighted_backward(c, need_opacity_grad, density); // (comes back with its gradient image)
    if (c->surface.reference_order()) return queue_backward_reference(c, need_opacity_grad, upstream);
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
// property of the separate kernels only, so a counting context takes those; so does a coverage context, whose kernels are the
// separate ones (image0 stored every time, whatever write_image says), and a context with a backdrop, whose backward walk reads
// the composite from image0, and a context with pixel weights, whose loss pass stands between the two walks.
int queue_forward_backward(s2d_ctx* c, bool need_opacity_grad, bool write_image)
{
    if ((c->cfg.flags & S2D_CFG_COUNT_PAIRS) || c->surface.reference_order() || coverage(c) || c->backdrop.set() || c->weights.set()) { // (reference order: its backward pass is a launch of its own)
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
    const bool fuse = c->reuse.adam_checks(c->fresh.lists());
    S2D_HIP(c, launch_adam(adam_args(c, flags, fuse), c->stream));
    if (fuse) S2D_HIP(c, c->reuse.check_queued());
    // The launch was told fresh.projection() as it stood BEFORE the step: only then may it leave the record and the check
    // of a splat it does not move as they are (adam_kernel); after any event that replaced parameters it projects and
    // checks every splat.
    c->fresh.invalidate(Stale::Projection);
    if (fuse) c->fresh.projected(); // (the step projected what it wrote: ListReuse::adam_checks)
    c->iterations++; // main.cpp:809
    c->reuse.step_queued();
    return S2D_OK;
}

int queue_status_read(s2d_ctx* c)
{
    S2D_HIP(c, hipMemcpyAsync(c->h_status, c->d_status, sizeof(DeviceStatus), hipMemcpyDeviceToHost, c->stream));
    return S2D_OK;
}

// The status word has been copied to h_status and the stream synchronised: act on it.
static int judge_status(s2d_ctx* c)
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
            c->fresh.invalidate(Stale::Frames);
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

// s2d_step (loss == nullptr) and s2d_step_loss: `iters` iterations queued in pieces of the rings' capacity, their squared
// errors (and loss totals) read back per piece, the status word judged once at the end.
int run_steps(s2d_ctx* c, int iters, uint32_t flags, const s2d_loss_config* loss, double* loss_out, double* mse_out)
{
    static_assert(TermRing::kCapacity == SqerrTrace::kCapacity, "one piece size for both rings");
    WalkFlags wf;
    if (int rc = parse_walk_flags(c, flags, true, &wf)) return rc;
    if (int rc = use_device(c)) return rc;
    // Under a weight plane s2d_step is s2d_step_loss with the squared error alone: the plane acts in the loss pass.
    static const s2d_loss_config mse_only = {(uint32_t)sizeof(s2d_loss_config), 1.0f, 0.0f, 0.0f};
    const bool weighted = c->weights.set();
    if (weighted)
        if (int rc = weights_refused_by_context(c, loss ? "s2d_step_loss" : "s2d_step")) return rc;
    if (weighted && !loss) loss = &mse_only;
    const TermRing& ring = current_ring(c); // (the plane cannot change within the call)
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
            sums.resize((size_t)ring.terms() * piece);
            S2D_HIP(c, ring.read(first_iter, piece, sums.data()));
        }
        if (mse_dst) S2D_HIP(c, c->trace.read(first_iter, piece, mse_dst));
        if (with_status)
            if (int rc = queue_status_read(c)) return rc;
        if (with_status || loss_out || mse_out) S2D_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; loss_out && k < piece; k++)
            loss_out[done + k] = loss_terms_of(c, ring.terms(), &sums[(size_t)ring.terms() * k], w).total;
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

// ---- events (s2d_sequence.h) -----------------------------------------------------------------------------------------
// One function per event, each doing all the event asks for.  Rules that are in none of them because no call site keeps
// them any more.  s2d_state.h: the id-indexed parameter and moment arrays are handed out by SplatState::current() only,
// which queues the write-back of a compact copy first; and a squared-error sum still waiting for its Adam launch is
// queued by SqerrTrace's own read() and settle(), the latter being what s2d_set_adam and s2d_init_splats call before they
// renumber the iterations.  s2d_context.h: a stamp that asked for new lists matches nothing once they are built, and every
// containment check has a sequence number of its own (ListReuse); the slots of an earlier backward walk are invalid in
// the next (PairScratch); which range's lists are in the buffers, and how far the last forward pass over ranges got
// (IndexRanges).

void target_replaced(s2d_ctx* c)
{
    c->fresh.target_set();
    c->fresh.invalidate(Stale::Frames);
    c->view.target_stale(); // (the views' own resampled target, s2d_step_view: derived from the one replaced)
}

// What image0 is composited over changed: the frames are stale; the projection and the lists depend on the splats alone.
void backdrop_replaced(s2d_ctx* c) { c->fresh.invalidate(Stale::Frames); }

// The weight plane of the losses was set, replaced or removed: the frames, the projection and the lists stand (no pass that
// produced them read it); the terms of the last loss pass are those of another loss and are forgotten.
void weights_replaced(s2d_ctx* c) { c->loss.record(-1, 0.0f, 0.0f, 0.0f); }

// Every splat is new (init / set_splats): the lists are none of theirs, and a non-finite event of the old ones no longer
// stops the queue.  (init also zeroes the gradients and restarts the counters, and asks for the arrays with
// discard_all(): every record, moments included, is new.)
int splats_replaced(s2d_ctx* c)
{
    S2D_HIP(c, c->state.written(true));
    S2D_HIP(c, hipMemcpyAsync(c->d_status, &kFreshStatus, sizeof(DeviceStatus), hipMemcpyHostToDevice, c->stream));
    c->fresh.invalidate(Stale::Lists);
    return S2D_OK;
}

// As rows_replaced(S2D_ROWS_SPLATS), over all rows.  Not Lists, and no fresh status word: this is the call of an
// optimisation loop outside the library, which moves every splat a little per call; a splat that left its rectangle gets
// its new lists from the containment check of the projection that follows.
int splats_replaced_from_device(s2d_ctx* c)
{
    S2D_HIP(c, c->state.written(true));
    c->fresh.invalidate(Stale::Projection);
    return S2D_OK;
}

// Some rows of `what` were written.  Parameters (with or without their moments): Projection, not Lists -- a row moves a
// splat a little, and the containment check of the projection that follows asks for new lists if it left its rectangle.
// Moments alone: nothing is stale, what is drawn depends on the parameters only.  Gradients: they are no state of a splat.
int rows_replaced(s2d_ctx* c, int32_t what)
{
    if (what != S2D_ROWS_GRADS) S2D_HIP(c, c->state.written(false));
    if (what == S2D_ROWS_SPLATS) c->fresh.invalidate(Stale::Projection);
    return S2D_OK;
}

int moments_replaced(s2d_ctx* c) // (nothing is stale: as the moments' rows)
{
    S2D_HIP(c, c->state.written(true));
    return S2D_OK;
}

// The lists hold the held splats only.  Splats arrived, or this is the first held set: the held ones are projected and
// the lists rebuilt before the next forward; so on the return to holding everything.  Departures alone leave lists that
// still cover every held splat.
void held_set_changed(s2d_ctx* c, bool had, bool has, bool added)
{
    if (has ? (added || !had) : had) c->fresh.invalidate(Stale::Lists);
}

// The alive set changed, in either direction: always the lists, and the projection with them.  Unlike a splat that left a
// rank's hold set -- which moved out of reach of the slab, so its old list entries cover nothing -- a row that died still
// covers its pixels through the entries it has, and would be drawn from them.
void alive_set_changed(s2d_ctx* c) { c->fresh.invalidate(Stale::Lists); }
