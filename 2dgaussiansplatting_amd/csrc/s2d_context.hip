// s2d_context.hip -- PairScratch, RasterSurface, IndexRanges and ListReuse (s2d_context.h).  Host code only; it queues memsets and copies.
#include "s2d_context.h"

#include <climits>
#include <cstdlib>

namespace s2d {

// (The two memsets are the blocking ones, on the null stream, which `stream` -- non-blocking -- does not wait for: what makes
// them safe is that hipMemset of device memory has completed when it returns.)
hipError_t PairScratch::create(Mode mode, const Geometry& g, size_t n, hipStream_t stream)
{
    release();
    mode_ = mode, stream_ = stream;
    if (reference_order()) {
        if (const char* e = getenv("S2D_REFERENCE_ORDER_MAX_BYTES")) {
            const unsigned long long v = strtoull(e, nullptr, 10);
            if (v > 0) max_bytes_ = v;
        }
        S2D_TRY(pixel_sqerr_.alloc((size_t)g.W * (size_t)(g.row_end - g.row_begin)));
    }
    if (deterministic() && !det_touched_) { // (per splat, zero between passes: it outlives a grid)
        S2D_TRY(det_touched_.alloc(n));
        S2D_TRY(hipMemset(det_touched_, 0, n * sizeof(uint32_t)));
    }
    S2D_TRY(tile_exec_.alloc((size_t)g.num_tiles));
    S2D_TRY(retire_hint_.alloc((size_t)g.num_tiles));
    return hipMemset(retire_hint_, 0xFF, (size_t)g.num_tiles * sizeof(uint32_t));
}

PairScratch::Grant PairScratch::admit(uint64_t need, uint64_t cap) const
{
    if (!reference_order()) return Grant{cap, 0, 0};
    const uint64_t per_slot = (uint64_t)kRefTermsStride * sizeof(float);
    if (cap * per_slot > max_bytes_) cap = std::max<uint64_t>(need, 1 << 16);
    if (cap * per_slot > max_bytes_) return Grant{0, cap, cap * per_slot};
    return Grant{cap, 0, 0};
}

void PairScratch::release()
{
    wave_masks_.release(), exec_list_.release(), det_data_.release(), stamp_.release(), ref_terms_.release();
    capacity_ = 0;
}

hipError_t PairScratch::alloc(uint64_t slots)
{
    const auto all = [&]() -> hipError_t {
        S2D_TRY(wave_masks_.alloc((size_t)slots * 4));
        S2D_TRY(exec_list_.alloc((size_t)slots));
        if (deterministic()) S2D_TRY(det_data_.alloc((size_t)slots * kDetStride));
        if (reference_order()) S2D_TRY(ref_terms_.alloc((size_t)slots * kRefTermsStride));
        if (mode_ == Mode::Atomic) return hipSuccess;
        S2D_TRY(stamp_.alloc((size_t)slots));
        return hipMemsetAsync(stamp_, 0, (size_t)slots * sizeof(uint32_t), stream_);
    };
    const hipError_t e = all();
    if (e == hipSuccess) capacity_ = slots;
    else release();
    return e;
}

void PairScratch::fill(RasterArgs* a, const TileRect* rects, const uint32_t* offsets, const uint32_t* counts, int first, int count) const
{
    a->wave_masks = wave_masks_, a->exec_list = exec_list_, a->tile_exec = tile_exec_, a->retire_hint = retire_hint_;
    if (deterministic()) a->det = DetGather{rects + first, offsets + first, counts + first, det_data_, stamp_, det_touched_ + first, 0u, count};
}

void PairScratch::backward_walk(RasterArgs* a)
{
    if (deterministic()) a->det.now = ++epoch_;
}

RefOrder PairScratch::reference_walk(const float* splats, const TileRect* rects, const uint32_t* offsets, const uint32_t* counts, int n)
{
    RefOrder ro;
    ro.splats = splats; ro.rects = rects; ro.offsets = offsets; ro.counts = counts; ro.n = n;
    ro.terms = ref_terms_; ro.stamp = stamp_; ro.capacity = (uint32_t)capacity_; ro.now = ++epoch_;
    ro.pixel_sqerr = pixel_sqerr_;
    return ro;
}

hipError_t RasterSurface::create(const Geometry& g, size_t n, bool generic, PairScratch::Mode mode, hipStream_t stream)
{
    if (created_) {
        S2D_TRY(hipStreamSynchronize(stream));
        created_ = false;
        lists_.reset(new TileLists()); // (the old grid's go before the new one's come; none of this grid until all of create() succeeded)
    }
    if (!proj_) {
        S2D_TRY(proj_.alloc(n));
        S2D_TRY(rects_.alloc(n));
        S2D_TRY(counts_.alloc(n));
        S2D_TRY(offsets_.alloc(n));
    }
    std::unique_ptr<TileLists> fresh(new TileLists()); // a failure keeps nothing of it: the next attempt may be for another grid and builder
    S2D_TRY(fresh->create(g, n, generic));
    S2D_TRY(scratch_.create(mode, g, n, stream));
    lists_ = std::move(fresh);
    g_ = g, stream_ = stream, created_ = true;
    return hipSuccess;
}

ProjectArgs RasterSurface::project_args(const float* splats, const uint8_t* held, int n, float margin) const
{
    ProjectArgs a;
    a.splats = splats; a.held = held; a.n = n; a.g = g_; a.margin = margin; a.proj = proj_; a.counts = counts_;
    a.row_counts = lists_->row_counts();
    a.check = ContainmentCheck{rects_, nullptr};
    return a;
}

hipError_t RasterSurface::count(int first, int n, uint32_t* scan_temp, uint64_t* pairs)
{
    return lists_->count(ListInput{rects_ + first, counts_ + first, offsets_ + first, first, n, scan_temp}, stream_, pairs);
}

hipError_t RasterSurface::ensure_pairs(uint64_t need, bool with_scratch, PairScratch::Grant* refused)
{
    const bool grow = lists_->capacity() == 0 || need > lists_->capacity(); // (the buffers exist from the first call on, also for no pair)
    const bool scratch = with_scratch && (grow || scratch_.capacity() != lists_->capacity());
    if (!grow && !scratch) return hipSuccess;
    if (need >= kMaxPairs) return hipErrorInvalidValue;
    uint64_t cap = grow ? pair_capacity(need) : lists_->capacity();
    if (scratch) {
        const PairScratch::Grant grant = scratch_.admit(grow ? need : cap, cap);
        if (!grant.slots) {
            if (refused) *refused = grant;
            return hipErrorOutOfMemory;
        }
        cap = grant.slots;
    }
    S2D_TRY(hipStreamSynchronize(stream_));
    if (grow) lists_->release_pairs();
    scratch_.release();
    if (grow) S2D_TRY(lists_->alloc_pairs(cap));
    if (!scratch) return hipSuccess;
    const hipError_t e = scratch_.alloc(cap);
    if (e != hipSuccess && grow) lists_->release_pairs(); // (capacity 0 is what is left if an allocation fails)
    return e;
}

void RasterSurface::fill(RasterArgs* a, int first, int count) const
{
    a->tile_off = lists_->tile_off(), a->list = lists_->list(), a->proj = proj_ + first;
    scratch_.fill(a, rects_, offsets_, counts_, first, count);
}

void IndexRanges::create(const Geometry& g, hipStream_t stream)
{
    g_ = g, stream_ = stream;
    if (const char* e = getenv("S2D_CHUNK_PAIRS")) { // (never beyond 32-bit positions)
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v > 0) budget_ = std::min<unsigned long long>(v, kMaxPairs - 1);
    }
}

hipError_t IndexRanges::plan(const uint32_t* counts_device, int n)
{
    std::vector<uint32_t> cnt((size_t)n);
    S2D_TRY(hipMemcpyAsync(cnt.data(), counts_device, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
    S2D_TRY(hipStreamSynchronize(stream_));
    cut_ = cut_index_ranges(cnt.data(), n, budget_);
    if (!state_) S2D_TRY(state_.alloc((size_t)g_.W * (size_t)(g_.row_end - g_.row_begin)));
    if (!alive_) S2D_TRY(alive_.alloc(1));
    return h_alive_.alloc(1, hipHostMallocDefault);
}

hipError_t IndexRanges::launching_forward(int k)
{
    walked_ = k + 1;
    return hipMemsetAsync(alive_, 0, sizeof(uint32_t), stream_);
}

hipError_t IndexRanges::any_alive(bool* alive)
{
    S2D_TRY(hipMemcpyAsync(h_alive_, alive_, sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
    S2D_TRY(hipStreamSynchronize(stream_));
    *alive = *(volatile uint32_t*)h_alive_ != 0u;
    return hipSuccess;
}

hipError_t ListReuse::create(int interval, float margin, hipStream_t stream)
{
    stream_ = stream;
    interval_ = interval > 0 ? interval : INT_MAX;
    margin_ = interval_ > 1 ? (margin > 0.0f ? margin : 2.0f) : 0.0f;
    S2D_TRY(ev_.create(hipEventDisableTiming));
    S2D_TRY(h_stamp_.alloc(16, hipHostMallocMapped));
    *h_stamp_ = 0;
    return hipSuccess;
}

hipError_t ListReuse::check_queued() { return hipEventRecord(ev_, stream_); }

hipError_t ListReuse::asked_for_lists(bool* asked)
{
    S2D_TRY(hipEventSynchronize(ev_));
    *asked = *(volatile int*)h_stamp_ == seq_;
    return hipSuccess;
}

} // namespace s2d
