// s2d_lists.h -- the per-tile lists of a context: every buffer that only a list build reads or writes, and the build.
// Host code only (s2d_lists.hip holds no kernel); the kernels it queues are those of s2d_scan_sort.hip, s2d_binning.hip
// and s2d_tilelists.hip.
#pragma once

#include "s2d_device.h"
#include "s2d_owned.h"

namespace s2d {

// What a build is lent: the per-splat arrays that other code reads as well (the Adam kernel's containment check, the
// deterministic gather, the range planner), from the build's first splat on, and the scan workspace of the context.
struct ListInput {
    const TileRect* rects;
    const uint32_t* counts;
    uint32_t* offsets;   // out: counts scanned (the deterministic gather addresses its slots through them)
    int first, n;        // the splats [first, first + n): `first` places the builder's own per-splat arrays
    uint32_t* scan_temp; // scan_temp_words(n) words
};

// Two builders with the same result (every tile's list ascending in splat index): the two-level one of
// s2d_tilelists.hip (images of up to kTlMaxColumns tile columns), and the generic one -- all (tile, splat) pairs
// emitted in splat order and radix-sorted by tile -- for wider images and on request.  A range's lists hold indices
// RELATIVE to its first splat, and so do the scanned offsets.
//
// A build has two phases, because its caller decides between them what to do with the pair count (render by index
// ranges, refuse, grow): count() queues the scans and a speculative emission and waits for the scans only; finish()
// runs the builder.  The pair buffers are sized by RasterSurface::ensure_pairs() (s2d_context.h) alone.
class S2D_LOCAL TileLists {
public:
    // n: splats (>= 1).  The pair buffers come with the first alloc_pairs().
    hipError_t create(const Geometry& g, size_t n, bool generic);
    void release_pairs();
    hipError_t alloc_pairs(uint64_t capacity);

    // Queues scans + emission, waits for the scans' event (the only wait of a build), returns the pair count of `in`
    // (saturated at 0xFFFFFFFF).  Nothing that an earlier finish() left is valid any more.
    hipError_t count(const ListInput& in, hipStream_t stream, uint64_t* pairs);
    // The pair count of the last count() fits capacity(): emits again if the pair buffers were replaced since, then builds
    // tile_off() and list().
    hipError_t finish(hipStream_t stream);

    const uint32_t* tile_off() const { return tile_off_; } // [tiles + 1]
    const uint32_t* list() const { return list_; }         // [pairs()], in one of the pair buffers
    uint64_t pairs() const { return pairs_; }              // of the last finished build
    uint64_t capacity() const { return capacity_; }
    uint64_t builds() const { return builds_; }            // finished builds, range builds included
    bool two_level() const { return two_level_; }
    uint32_t* row_counts() const { return row_counts_; }   // per splat, for launch_project mode 0; null: generic builder

private:
    hipError_t emit(hipStream_t stream);

    // A scan's sum: the device word, and a host-mapped one that the scan's last kernel writes itself (no copy engine
    // between two kernels), complete once ev_total_ is.
    struct Total {
        DevBuf<uint32_t> dev;
        HostBuf<uint32_t> host;
        uint64_t read() const { return *(volatile uint32_t*)host; }
    };
    Geometry g_{};
    bool two_level_ = false;
    Total pair_total_, entry_total_; // (tile, splat) pairs; (splat, tile row) entries of the two-level builder
    Event ev_total_;                 // recorded behind the scans
    DevBuf<uint32_t> keys_[2], vals_[2], sort_temp_; // pair-sized: emission -> [0], the sorts ping-pong
    uint64_t capacity_ = 0;
    DevBuf<uint32_t> tile_off_;
    DevBuf<uint32_t> tile_first_;  // generic: per tile id (padded to a power of two) the position of its first pair, + chunk minima
    DevBuf<uint32_t> row_counts_;  // two-level, per splat: tile rows its rectangle covers
    DevBuf<uint32_t> row_offsets_; // ... scanned
    DevBuf<uint32_t> row_off_;     // [tiles_y + 1]: where each tile row's entries begin
    DevBuf<uint32_t> chunk_base_;  // [tiles_y + 1]
    DevBuf<uint32_t> tl_hist_;     // per (row, column, chunk) counts + scan workspace; grows with the entries
    const uint32_t* list_ = nullptr;
    ListInput in_{};               // of the build in progress
    uint64_t counted_ = 0;         // its pair count
    bool emitted_ = false;         // ... and its emission is in the pair buffers (they were not replaced since)
    uint64_t pairs_ = 0, builds_ = 0;
};

} // namespace s2d
