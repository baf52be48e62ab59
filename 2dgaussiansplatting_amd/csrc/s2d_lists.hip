// s2d_lists.hip -- TileLists (s2d_lists.h): project has run with mode 0; count scan -> emit -> sort -> tile offsets.
// Host code only.
#include "s2d_lists.h"

#include <initializer_list>

namespace s2d {

static int key_bits_for(int keys)
{
    int bits = 0;
    while ((1 << bits) < keys) bits++;
    return bits;
}

hipError_t TileLists::create(const Geometry& g, size_t n, bool generic)
{
    g_ = g;
    two_level_ = g.tiles_x <= kTlMaxColumns && !generic;
    for (Total* t : {&pair_total_, &entry_total_}) {
        S2D_TRY(t->dev.alloc(1));
        S2D_TRY(t->host.alloc(16, hipHostMallocMapped)); // (a 64-byte line of its own)
    }
    S2D_TRY(ev_total_.create(hipEventDisableTiming));
    S2D_TRY(tile_off_.alloc((size_t)g.num_tiles + 1));
    S2D_TRY(tile_first_.alloc(((size_t)1 << key_bits_for(g.num_tiles)) + tile_first_temp_words(g.num_tiles)));
    if (two_level_) {
        S2D_TRY(row_counts_.alloc(n));
        S2D_TRY(row_offsets_.alloc(n));
        S2D_TRY(row_off_.alloc((size_t)g.tiles_y + 1));
        S2D_TRY(chunk_base_.alloc((size_t)g.tiles_y + 1));
    }
    return hipSuccess;
}

void TileLists::release_pairs()
{
    for (int k = 0; k < 2; k++) keys_[k].release(), vals_[k].release();
    sort_temp_.release();
    capacity_ = 0;
    emitted_ = false;
}

hipError_t TileLists::alloc_pairs(uint64_t capacity)
{
    for (int k = 0; k < 2; k++) {
        S2D_TRY(keys_[k].alloc(capacity));
        S2D_TRY(vals_[k].alloc(capacity));
    }
    S2D_TRY(sort_temp_.alloc(sort_temp_words((int64_t)capacity)));
    capacity_ = capacity;
    return hipSuccess;
}

// (never writes past the buffers' capacity; there are never more row entries than pairs: the pair buffers hold them)
hipError_t TileLists::emit(hipStream_t stream)
{
    emitted_ = true;
    if (two_level_)
        return launch_emit_row_entries(in_.rects, row_offsets_ + in_.first, row_counts_ + in_.first, in_.n, keys_[0], vals_[0],
                                       (uint32_t)capacity_, stream);
    return launch_emit_pairs(in_.rects, in_.offsets, in_.counts, in_.n, g_, keys_[0], vals_[0], (uint32_t)capacity_, stream);
}

hipError_t TileLists::count(const ListInput& in, hipStream_t stream, uint64_t* pairs)
{
    in_ = in;
    list_ = nullptr;
    S2D_TRY(exclusive_scan_u32(in.counts, in.offsets, in.n, in.scan_temp, pair_total_.dev, stream, pair_total_.host));
    if (two_level_)
        S2D_TRY(exclusive_scan_u32(row_counts_ + in.first, row_offsets_ + in.first, in.n, in.scan_temp, entry_total_.dev, stream,
                                   entry_total_.host));
    S2D_TRY(hipEventRecord(ev_total_, stream));
    // The emission needs the offsets, not the totals: queue it behind the scans and wait for the SCANS only, so the host
    // reads the totals and queues the rest while the emission runs instead of the device idling through the host's
    // round trip (~30 us per build).  Only when the pairs outgrow the buffers (rare: they are sized with a quarter to
    // spare) does finish() queue it again.
    S2D_TRY(emit(stream));
    S2D_TRY(hipEventSynchronize(ev_total_));
    *pairs = counted_ = pair_total_.read(); // saturates at 0xFFFFFFFF instead of wrapping (scan_top_kernel)
    return hipSuccess;
}

hipError_t TileLists::finish(hipStream_t stream)
{
    const uint64_t total = counted_;
    if (!emitted_) S2D_TRY(emit(stream));
    uint32_t *k_out = nullptr, *v_out = nullptr;
    if (two_level_) {
        const uint64_t entries = entry_total_.read();
        const size_t need = tl_workspace_words(entries, g_.tiles_x, g_.tiles_y);
        if (need > tl_hist_.capacity()) {
            S2D_TRY(hipStreamSynchronize(stream));
            S2D_TRY(tl_hist_.alloc(need + need / 4 + 4096));
        }
        const int row_bits = key_bits_for(g_.tiles_y);
        if (row_bits > 0) { // level 1: the entries by tile row, and where every row begins
            // (sorted keys written out and compared: with only tiles_y distinct keys the last pass's atomicMin per (block,
            // key) would pile thousands of atomics on each of a few hundred words)
            S2D_TRY(sort_pairs_u32(keys_[0], vals_[0], keys_[1], vals_[1], (int64_t)entries, row_bits, sort_temp_, &k_out, &v_out,
                                   nullptr, stream));
            S2D_TRY(launch_tile_offsets(k_out, (uint32_t)entries, g_.tiles_y, row_off_, stream, (1u << kTlRowBits) - 1u));
        } else { // one tile row: the emission order is the row's order
            const uint32_t two[2] = {0u, (uint32_t)entries};
            S2D_TRY(hipMemcpyAsync(row_off_, two, sizeof(two), hipMemcpyHostToDevice, stream));
            S2D_TRY(hipStreamSynchronize(stream)); // (`two` lives on this stack frame)
            v_out = vals_[0];
            k_out = keys_[0];
        }
        // level 2: every row's entries by column, straight into the lists (the value buffer the sort finished with is free)
        uint32_t* const list = v_out == vals_[0] ? vals_[1] : vals_[0];
        S2D_TRY(launch_tile_lists_from_rows(v_out, k_out, entries, row_off_, g_, chunk_base_, tl_hist_, tile_off_, list, stream));
        list_ = list;
    } else {
        const int key_bits = key_bits_for(g_.num_tiles);
        if (key_bits > 0) {
            // the last radix pass records where each tile's pairs begin instead of writing the sorted keys out
            S2D_TRY(hipMemsetAsync(tile_first_, 0xFF, ((size_t)1 << key_bits) * sizeof(uint32_t), stream));
            S2D_TRY(sort_pairs_u32(keys_[0], vals_[0], keys_[1], vals_[1], (int64_t)total, key_bits, sort_temp_, &k_out, &v_out,
                                   tile_first_, stream));
            S2D_TRY(launch_tile_offsets_from_first(tile_first_, g_.num_tiles, (uint32_t)total, tile_first_ + ((size_t)1 << key_bits),
                                                   tile_off_, stream));
        } else { // a single tile: nothing to sort
            S2D_TRY(sort_pairs_u32(keys_[0], vals_[0], keys_[1], vals_[1], (int64_t)total, key_bits, sort_temp_, &k_out, &v_out,
                                   nullptr, stream));
            S2D_TRY(launch_tile_offsets(k_out, (uint32_t)total, g_.num_tiles, tile_off_, stream));
        }
        list_ = v_out;
    }
    emitted_ = false; // (the sorts have used the buffers)
    pairs_ = total;
    builds_++;
    return hipSuccess;
}

} // namespace s2d
