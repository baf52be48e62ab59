// s2d_state.hip -- SplatState and SqerrTrace (s2d_state.h).  Host code only; the kernels it queues are those of
// s2d_halo.hip (compact copies, the held set) and s2d_raster.hip (sqerr_finalize).
#include "s2d_state.h"

#include <cstdlib>

#include "s2d_alive.h"

namespace s2d {

hipError_t SplatState::create(int n, hipStream_t stream)
{
    n_ = n, stream_ = stream;
    const size_t rows = std::max<size_t>((size_t)n, 1); // >= 1 so that n == 0 still has buffers
    if (const char* e = getenv("S2D_COMPACT_HELD")) compact_enabled_ = atoi(e) != 0;
    S2D_TRY(splats_.alloc(rows * 9));
    S2D_TRY(adams_.alloc(rows * 18));
    S2D_TRY(dormant_.alloc(rows));
    S2D_TRY(hipMemsetAsync(splats_, 0, rows * 9 * sizeof(float), stream));
    S2D_TRY(hipMemsetAsync(adams_, 0, rows * 18 * sizeof(float), stream));
    return hipMemsetAsync(dormant_, 0, rows, stream);
}

// Bring the id-indexed arrays up to date ...
hipError_t SplatState::flush()
{
    if (!live_ || !dirty_) return hipSuccess;
    S2D_TRY(launch_compact_copy(splats_, 9, held_ids_, held_count_, n_, csplats_, false, stream_));
    S2D_TRY(launch_compact_copy(adams_, 18, held_ids_, held_count_, n_, cadams_, false, stream_));
    dirty_ = false;
    return hipSuccess;
}

// ... and make the compact copy afresh from them (the held set, or the arrays, changed from outside).
hipError_t SplatState::load()
{
    live_ = dirty_ = false;
    if (!held_ || !compact_enabled_ || n_ <= 0) return hipSuccess;
    if (!csplats_) {
        S2D_TRY(csplats_.alloc((size_t)n_ * 9));
        S2D_TRY(cadams_.alloc((size_t)n_ * 18));
    }
    S2D_TRY(launch_compact_copy(splats_, 9, held_ids_, held_count_, n_, csplats_, true, stream_));
    S2D_TRY(launch_compact_copy(adams_, 18, held_ids_, held_count_, n_, cadams_, true, stream_));
    live_ = true;
    return hipSuccess;
}

hipError_t SplatState::current(Arrays* out)
{
    *out = Arrays{splats_, adams_};
    return flush();
}

hipError_t SplatState::written(bool all_rows)
{
    if (all_rows || live_) S2D_TRY(load());
    return n_ > 0 ? hipMemsetAsync(dormant_, 0, (size_t)n_, stream_) : hipSuccess;
}

hipError_t SplatState::commit(const uint32_t* masks, int rank, uint32_t* scan_temp)
{
    S2D_TRY(flush()); // the id-indexed arrays take over while the held set changes
    live_ = false;
    if (!masks) { // (the caller has made this context's copy complete again)
        if (held_) S2D_TRY(hipStreamSynchronize(stream_));
        held_.release(), held_ids_.release(), held_work_.release(), held_count_.release();
        kind_ = Subset::None;
        return hipSuccess;
    }
    kind_ = Subset::Slab;
    if (!held_) {
        S2D_TRY(held_.alloc((size_t)n_));
        S2D_TRY(held_ids_.alloc((size_t)n_));
        S2D_TRY(held_work_.alloc((size_t)n_));
        S2D_TRY(held_count_.alloc(4));
    }
    S2D_TRY(launch_halo_commit(masks, n_, rank, held_, held_ids_, held_count_, held_work_, scan_temp, stream_));
    return load();
}

hipError_t SplatState::list_alive(float* grads, uint32_t* scan_temp)
{
    if (n_ <= 0) return hipMemsetAsync(held_count_, 0, sizeof(uint32_t), stream_);
    S2D_TRY(launch_alive_flags(held_, 0, n_, held_, held_work_, grads, stream_));
    S2D_TRY(exclusive_scan_u32(held_work_, held_work_, n_, scan_temp, held_count_, stream_)); // held_count_ = number of alive rows
    return launch_held_ids(held_, held_work_, n_, held_ids_, stream_);
}

hipError_t SplatState::begin_alive(uint8_t** flags, uint32_t* scan_temp)
{
    S2D_TRY(flush()); // the id-indexed arrays take over while the set changes
    live_ = false;
    alive_count_ = -1;
    if (!held_) {
        S2D_TRY(held_.alloc((size_t)n_));
        S2D_TRY(held_ids_.alloc((size_t)n_));
        S2D_TRY(held_work_.alloc((size_t)n_));
        S2D_TRY(held_count_.alloc(4));
        if (n_ > 0) S2D_TRY(hipMemsetAsync(held_, 1, (size_t)n_, stream_)); // without a set every row is alive
        S2D_TRY(list_alive(nullptr, scan_temp)); // (valid from here on, whatever becomes of the edit)
    }
    kind_ = Subset::Alive;
    *flags = held_;
    return hipSuccess;
}

hipError_t SplatState::finish_alive(float* grads, uint32_t* scan_temp)
{
    S2D_TRY(list_alive(grads, scan_temp));
    return load();
}

hipError_t SplatState::clear_alive()
{
    if (kind_ != Subset::Alive) return hipSuccess;
    S2D_TRY(flush());
    live_ = false;
    S2D_TRY(hipStreamSynchronize(stream_));
    held_.release(), held_ids_.release(), held_work_.release(), held_count_.release();
    kind_ = Subset::None;
    alive_count_ = -1;
    return hipSuccess;
}

hipError_t SplatState::alive_count(int* out)
{
    if (kind_ != Subset::Alive) {
        *out = n_;
        return hipSuccess;
    }
    if (alive_count_ < 0) {
        uint32_t count = 0;
        S2D_TRY(hipMemcpyAsync(&count, held_count_, sizeof(count), hipMemcpyDeviceToHost, stream_));
        S2D_TRY(hipStreamSynchronize(stream_));
        alive_count_ = (int)std::min<uint32_t>(count, (uint32_t)n_);
    }
    *out = alive_count_;
    return hipSuccess;
}

SplatState::AdamStep SplatState::adam_step()
{
    const bool compact = live_ && held_ids_ != nullptr;
    if (compact) dirty_ = true;
    return AdamStep{compact ? Arrays{csplats_, cadams_} : Arrays{splats_, adams_}, compact, held_ids_, held_count_, dormant_};
}

hipError_t SqerrTrace::create(int num_tiles, int n, const DeviceStatus* status, hipStream_t stream)
{
    num_tiles_ = num_tiles, adam_blocks_ = (n + 255) / 256, status_ = status, stream_ = stream;
    S2D_TRY(tile_sqerr_.alloc((size_t)num_tiles + kSqerrScratchDoubles));
    S2D_TRY(ring_.alloc(kCapacity));
    S2D_TRY(pinned_.alloc(kPinned, hipHostMallocDefault));
    S2D_TRY(hipMemsetAsync(tile_sqerr_ + num_tiles, 0, kSqerrScratchDoubles * sizeof(double), stream)); // (what sqerr_reduce expects)
    return hipMemsetAsync(ring_, 0, (size_t)kCapacity * sizeof(double), stream);
}

SqerrBy SqerrTrace::plan(bool whole_iteration, bool fused_launch) const
{
    // The Adam launch does it on the way where it has a workgroup per chunk of tile errors -- a 4-workgroup launch would
    // walk 16 chunks each; 535x426 / 50 k measured 6.9 % slower with the in-raster sum.  (Such a launch has splats: a
    // context without any, whose Adam step queues nothing, never leaves a sum waiting.)
    if (whole_iteration && adam_blocks_ >= kSqerrChunks) return SqerrBy::NextAdam;
    // Few tiles: the fused launch's last tile adds them up itself.  A scene that went to index ranges never ran it.
    if (whole_iteration && fused_launch && num_tiles_ <= kSqerrSmallTiles) return SqerrBy::PassItself;
    return SqerrBy::OwnKernel;
}

SqerrJob SqerrTrace::job(int iteration) const
{
    return SqerrJob{tile_sqerr_, num_tiles_, ring_ + iteration % kCapacity, tile_sqerr_ + num_tiles_};
}

hipError_t SqerrTrace::record(int iteration, SqerrBy by)
{
    if (by == SqerrBy::NoLoss) return hipSuccess; // (a sum still waiting stays as the last pass with a loss left it)
    last_ = iteration;
    waiting_ = by != SqerrBy::PassItself && by != SqerrBy::LossPass;
    return by == SqerrBy::OwnKernel ? settle() : hipSuccess;
}

SqerrJob SqerrTrace::take_for_adam()
{
    const bool had = waiting_;
    waiting_ = false;
    return had ? job(last_) : SqerrJob{nullptr, 0, nullptr, nullptr};
}

hipError_t SqerrTrace::settle()
{
    if (!waiting_) return hipSuccess;
    waiting_ = false;
    return launch_sqerr_finalize(job(last_), status_, last_, stream_);
}

hipError_t SqerrTrace::read(int first, int count, double* out)
{
    S2D_TRY(settle());
    for (int got = 0; got < count;) {
        const int slot = (first + got) % kCapacity, run = std::min(count - got, kCapacity - slot);
        S2D_TRY(hipMemcpyAsync(out + got, ring_ + slot, (size_t)run * sizeof(double), hipMemcpyDeviceToHost, stream_));
        got += run;
    }
    return hipSuccess;
}

hipError_t DensityStats::next_pass(float** out)
{
    if (!buf_) {
        S2D_TRY(buf_.alloc((size_t)n_ * 3));
        S2D_TRY(hipMemsetAsync(buf_, 0, buf_.capacity() * sizeof(float), stream_));
    }
    passes_++;
    *out = buf_;
    return hipSuccess;
}

hipError_t DensityStats::reset()
{
    passes_ = 0;
    return buf_ ? hipMemsetAsync(buf_, 0, buf_.capacity() * sizeof(float), stream_) : hipSuccess;
}

} // namespace s2d
