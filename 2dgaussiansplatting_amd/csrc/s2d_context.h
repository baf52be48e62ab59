// s2d_context.h -- four owners of context state whose rules used to be kept by hand across the API file (now s2d_sequence.hip): the raster's
// scratch that is sized like the tile lists (PairScratch), everything a raster grid derives from a set of records (RasterSurface),
// the cut and the progress of a pass over index ranges (IndexRanges), and the schedule and the stamps of list re-use (ListReuse).
// Host code only (s2d_context.hip holds no kernel); each works on the context's stream, handed over once.
#pragma once

#include <memory>
#include <vector>

#include "s2d_device.h"
#include "s2d_lists.h"
#include "s2d_owned.h"
#include "s2d_ranges.h"

namespace s2d {

// Everything sized by pair capacity outside TileLists, and what rides with it: the forward -> backward hand-over of every
// mode, and the slots of the two modes that replace float atomics.  Both modes number their slots alike (offsets[splat] +
// position of the tile in the splat's binned rectangle) and stamp a slot with the epoch of the backward walk that wrote
// it, so one stamp array and one epoch counter serve whichever is on; a slot of an earlier walk, or one never written
// (stamp 0), matches no epoch handed out here.  The epoch counts on for as long as the object lives, whatever becomes of the
// slots (alloc() clears their stamps, create() for another grid releases them): no stamp meets an epoch that restarted.
class S2D_LOCAL PairScratch {
public:
    enum class Mode {
        Atomic,
        Deterministic,  // S2D_CFG_DETERMINISTIC: partial gradients into slots, a gather adds them in slot order
        ReferenceOrder, // S2D_CFG_REFERENCE_ORDER: per-pixel terms into slots, added in the reference's order (replaces the above)
    };
    // n: splats (>= 1); the per-tile and per-splat words are allocated and set here, the pair-sized arrays by alloc().
    // Reference order reads S2D_REFERENCE_ORDER_MAX_BYTES, the bound on its term scratch (default 32 GiB).
    // Again, for another grid of the same splats (the caller has made the stream idle): the pair-sized arrays go.
    hipError_t create(Mode mode, const Geometry& g, size_t n, hipStream_t stream);
    bool deterministic() const { return mode_ == Mode::Deterministic; }
    bool reference_order() const { return mode_ == Mode::ReferenceOrder; }

    // May the scratch have `cap` slots, `need` of them being required?  slots: what to allocate -- `cap`, or `need` without
    // headroom where only that fits the byte bound (no headroom rather than no context) -- or 0: refused, `bytes` being
    // what `refused` slots would take of max_bytes().
    struct Grant {
        uint64_t slots, refused, bytes;
    };
    Grant admit(uint64_t need, uint64_t cap) const;
    uint64_t max_bytes() const { return max_bytes_; }
    uint64_t capacity() const { return capacity_; } // slots allocated: 0, or what the lists have room for
    void release();
    hipError_t alloc(uint64_t slots); // stamps cleared (queued); capacity 0 is what is left if an allocation fails

    // The scratch's part of a raster pass over the lists of the splats [first, first + count): the hand-over, and in
    // deterministic mode the gather over those splats' slots (per-splat arrays from `first` on).  det.now stays 0, no
    // gather, until backward_walk().
    void fill(RasterArgs* a, const TileRect* rects, const uint32_t* offsets, const uint32_t* counts, int first, int count) const;
    // The pass gets a backward walk: a fresh epoch for its slots (those of earlier walks become invalid).
    void backward_walk(RasterArgs* a);
    // The same for a reference-order backward pass, whose slots go with a record of its own.
    RefOrder reference_walk(const float* splats, const TileRect* rects, const uint32_t* offsets, const uint32_t* counts, int n);
    float* pixel_sqerr() const { return pixel_sqerr_; } // reference order, [pixels of the slab]

private:
    Mode mode_ = Mode::Atomic;
    hipStream_t stream_ = nullptr;
    uint64_t capacity_ = 0;
    DevBuf<unsigned long long> wave_masks_; // 4 x u64 per listed pair (written per executed pair): forward -> backward lane masks
    DevBuf<uint32_t> exec_list_;            // per listed pair: splat indices of a tile's executed entries, compacted
    DevBuf<uint32_t> tile_exec_;            // [tiles]: how many entries the tile's last forward walk handed over
    DevBuf<uint32_t> retire_hint_;          // [tiles]: list position at which the tile retired in the last launch (0xFFFFFFFF:
                                            // unknown); a hint for batch sizes only, so it survives list rebuilds and new
                                            // splats (measured better than a reset)
    DevBuf<float> det_data_;                // deterministic: [capacity][kDetStride] per-(tile, splat) partial gradients
    DevBuf<uint32_t> det_touched_;          // deterministic: [n], which of a splat's slots the current pass wrote (zero between passes)
    DevBuf<uint32_t> stamp_;                // either slot mode: [capacity]
    uint32_t epoch_ = 0;                    // stamps handed out so far (monotone; 0 = never)
    uint64_t max_bytes_ = 32ull << 30;
    DevBuf<float> ref_terms_;               // reference order: [capacity][kRefTermsStride]
    DevBuf<float> pixel_sqerr_;
};

// Everything a raster grid derives from a set of n x 9 records: the per-splat arrays the projection writes and a list build
// scans, the per-tile lists, and the raster's scratch.  The context has one for its training image, with its scratch from
// the start; its views share one (ViewScratch, s2d_view.h), whose scratch arrives with the first gradient pass.
class S2D_LOCAL RasterSurface {
public:
    // n: splats (>= 1).  Again, for a grid of another size: the per-splat arrays stay, what is per tile and per pair goes, behind an idle stream.
    hipError_t create(const Geometry& g, size_t n, bool generic, PairScratch::Mode mode, hipStream_t stream);
    bool allocated() const { return created_ || proj_; }
    bool on(const Geometry& g) const { return created_ && g.W == g_.W && g.H == g_.H; } // ... for a grid of this size

    // Mode 0 of the projection over these arrays: rectangles inflated by `margin`, pair and row counts for a build.
    ProjectArgs project_args(const float* splats, const uint8_t* held, int n, float margin) const;
    // A list build over the splats [first, first + n) (TileLists::count / finish; scan_temp: scan_temp_words(n) words, lent).
    hipError_t count(int first, int n, uint32_t* scan_temp, uint64_t* pairs);
    hipError_t finish() { return lists_->finish(stream_); }
    // The one place where pair-sized memory grows: room for `need` (< kMaxPairs) pairs in the lists, and with_scratch: a scratch
    // of the lists' capacity (it has that or none at all).  Nothing is allocated when both are there.  Otherwise admit() first -- a
    // refusal (hipErrorOutOfMemory, *refused says why) comes before anything is released or launched -- then, with the stream idle,
    // what is replaced goes before the first is allocated again.
    hipError_t ensure_pairs(uint64_t need, bool with_scratch, PairScratch::Grant* refused = nullptr);

    // What a raster pass over the lists of the splats [first, first + count) works on: lists, records and PairScratch::fill.
    void fill(RasterArgs* a, int first, int count) const;
    void backward_walk(RasterArgs* a) { scratch_.backward_walk(a); } // a fresh epoch for the pass's slots
    RefOrder reference_walk(const float* splats, int n) { return scratch_.reference_walk(splats, rects_, offsets_, counts_, n); }

    const TileLists& lists() const { return *lists_; }
    ProjRec* proj() const { return proj_; }
    TileRect* rects() const { return rects_; }
    uint32_t* counts() const { return counts_; }
    uint32_t* offsets() const { return offsets_; }
    bool deterministic() const { return scratch_.deterministic(); }
    bool reference_order() const { return scratch_.reference_order(); }
    float* pixel_sqerr() const { return scratch_.pixel_sqerr(); }
    uint64_t max_bytes() const { return scratch_.max_bytes(); }

private:
    Geometry g_{};
    hipStream_t stream_ = nullptr;
    DevBuf<ProjRec> proj_;
    DevBuf<TileRect> rects_;
    DevBuf<uint32_t> counts_, offsets_;
    std::unique_ptr<TileLists> lists_{new TileLists()}; // (replaced whole with the grid)
    PairScratch scratch_;
    bool created_ = false;
};

// Index-range ("chunked") rendering: when the (tile, splat) pairs of a scene exceed budget() -- at the latest 2^32 - 65536,
// what 32-bit list positions can address -- the splats are cut into consecutive index ranges of at most that many pairs
// (cut_index_ranges, s2d_ranges.h), and the lists of one range at a time are built and walked front to back.  This owner
// keeps the cut, the per-pixel (colour, T) carried from range to range, and how far the last forward pass got; building
// and launching are its caller's.
class S2D_LOCAL IndexRanges {
public:
    // Reads S2D_CHUNK_PAIRS: pairs per range (tests force the path on small scenes; default 2^30).
    void create(const Geometry& g, hipStream_t stream);
    uint64_t budget() const { return budget_; }
    bool active() const { return !cut_.empty(); } // the last forward pass went over ranges
    void clear() { cut_.clear(); }                // one set of lists again
    // Cuts the n splats by their pair counts (device; one copy and one wait) and makes sure of the carry buffers.
    hipError_t plan(const uint32_t* counts_device, int n);
    int count() const { return (int)cut_.size() - 1; }
    int first(int k) const { return cut_[(size_t)k]; }
    int size(int k) const { return cut_[(size_t)k + 1] - cut_[(size_t)k]; }
    // Which range's lists are in the buffers (a range's lists are walked once and replaced by the next range's).
    bool built(int k) const { return built_ == k; }
    void set_built(int k) { built_ = k; } // -1: none
    // A forward pass starts; range k of it is about to be launched (the alive word is cleared, queued); how many it walked.
    void begin_forward() { walked_ = 0, built_ = -1; }
    hipError_t launching_forward(int k);
    int walked() const { return walked_; }
    // Is any pixel of the slab still above the throughput cut-off behind the range just launched?  (4 bytes and a wait.)
    hipError_t any_alive(bool* alive);
    // The carry's part of a raster pass over range k (k < 0: no range, the pass uses none of it).
    void fill(RasterArgs* a, int k) const { a->state = state_, a->any_alive = alive_, a->first = k == 0; }

private:
    Geometry g_{};
    hipStream_t stream_ = nullptr;
    uint64_t budget_ = 1ull << 30;
    std::vector<int> cut_;       // range k = splats [cut_[k], cut_[k+1]); empty: one set of lists
    int walked_ = 0;             // ranges the last forward pass walked before every pixel was saturated
    int built_ = -1;
    DevBuf<float4> state_;       // per pixel of the slab: (r, g, b, T); allocated by the first plan()
    DevBuf<uint32_t> alive_;     // != 0: some pixel is still above the throughput cut-off after this range
    HostBuf<uint32_t> h_alive_;  // ... read back between two ranges
};

// List re-use (rebin_interval > 1): lists built from rectangles inflated by margin() stay in use until a containment check
// finds a splat outside its rectangle, or the interval has passed.  A check is a kernel (the projection in mode 1, or the
// Adam launch) that stamps a device word and a host-mapped word with the check's sequence number on failure; the raster
// launch behind it is queued optimistically with the same number as abort_stamp() and does nothing on a match, and the host
// reads its word after that launch.  Checks and rebuilds share the one sequence, counted here only: after a rebuild a stamp
// that asked for it matches nothing any more.  (Both stamp words start at 0, the sequence at 1: nothing matches before a
// check.)
class S2D_LOCAL ListReuse {
public:
    // interval <= 0: rebuild on a failed check only; margin <= 0: 2 pixels (none without re-use).
    hipError_t create(int interval, float margin, hipStream_t stream);
    float margin() const { return margin_; }
    bool rebuild_scheduled(bool lists_valid) const { return !lists_valid || interval_ <= 1 || since_ >= interval_; }
    bool adam_checks(bool lists_valid) const { return lists_valid && interval_ > 1; } // ... and projects what it wrote
    // A check is about to be queued: its record, with the next sequence number.
    ContainmentCheck next_check(TileRect* rects, DeviceStatus* status) { return ContainmentCheck{rects, status, ++seq_, h_stamp_}; }
    // The record of a launch that takes one but runs no check (its stamp is the latest check's, and goes unused).
    ContainmentCheck idle_check(TileRect* rects, DeviceStatus* status) const { return ContainmentCheck{rects, status, seq_, h_stamp_}; }
    hipError_t check_queued(); // ... behind which the event is recorded
    int abort_stamp() const { return seq_; }
    // Did the latest check ask for new lists?  Waits for the checking kernel (not for what was queued behind it).
    hipError_t asked_for_lists(bool* asked);
    void lists_rebuilt() { since_ = 0, seq_++; } // they cover the current parameters: outstanding stamps are retired
    void step_queued() { since_++; }

private:
    hipStream_t stream_ = nullptr;
    Event ev_;               // recorded behind the kernel that ran the latest check
    HostBuf<int> h_stamp_;   // host-mapped copy of the stamp (written by that kernel, read after ev_)
    int seq_ = 1;
    int interval_ = 1, since_ = 0;
    float margin_ = 0.0f;
};

} // namespace s2d
