// s2d_state.h -- two owners of context state whose rules used to be kept by hand at every call site: where a splat's
// parameters and moments live (SplatState), and who sums a pass's squared error into which ring slot (SqerrTrace).
// Host code only (s2d_state.hip holds no kernel); each works on the context's stream, handed over once.
#pragma once

#include "s2d_device.h"
#include "s2d_owned.h"

namespace s2d {

// Parameters, Adam moments and the subset of the splats that takes part: the held set of slab ownership (s2d_halo_commit), or
// the alive set of a single context (s2d_set_alive, s2d_prune, s2d_grow).  One context has one kind at a
// time, kind() says which.  Both are the same machinery: flags that project_kernel reads, an ascending id list and compact
// record copies for the Adam kernels.  With a held set the Adam step touches only the splats the
// rank holds -- a seventh of them at eight ranks, scattered through the id-indexed arrays (36- and 72-byte records, a cache
// line or two each).  Their records are therefore kept in compact arrays in the order of held_ids, which the Adam kernel
// reads and writes in whole lines, and which run ahead of the id-indexed arrays between two readers of those.  Nobody
// outside gets the id-indexed pointers without the write-back having been queued: current() is the only way to them.
class S2D_LOCAL SplatState {
public:
    struct Arrays {
        float* splats; // n x 9, by splat id (AoS, the reference's layouts)
        float* adams;  // n x 18
    };
    struct AdamStep {
        Arrays arrays; // compact: record h is splat held_ids[h]'s; otherwise the id-indexed ones
        bool compact;
        const uint32_t *held_ids, *held_count; // the held splats, ascending, *held_count of them; null: all
        uint8_t* dormant; // [n]: 1 = all of the splat's moments are +0, bit for bit (adam_kernel keeps it; written() clears it)
    };

    hipError_t create(int n, hipStream_t stream); // zeroed (queued); S2D_COMPACT_HELD=0 turns the compact copy off (A/B)
    // The id-indexed arrays with everything queued so far in them, for reading or for writing some of it.
    hipError_t current(Arrays* out);
    // The same arrays for a caller that replaces EVERY record, moments included, and says written(true) then: nothing of
    // a compact copy that is ahead of them is worth writing back first.
    Arrays discard_all() { return Arrays{splats_, adams_}; }
    // Records have been written (queued) from outside the Adam kernel, all of them or some rows: the compact copy is made
    // again -- rows of held splats may be among them -- and nothing is known to be dormant any more (the next step of every
    // splat is a full one, which also applies the constraints to whatever was loaded).
    hipError_t written(bool all_rows);
    // s2d_halo_commit: the held set becomes bit `rank` of masks[] (nullptr: every splat again, the buffers go).
    hipError_t commit(const uint32_t* masks, int rank, uint32_t* scan_temp);
    const uint8_t* held() const { return held_; } // [n]: 1 = this rank holds (updates) the splat, or the row is alive; nullptr: all
    enum class Subset { None, Slab, Alive };
    Subset kind() const { return kind_; } // whose set held() is
    // The alive set, the second way to a subset.  An edit is three steps on the stream: begin_alive() -- the id-indexed arrays
    // take over, the flag bytes exist (all ones when there was no set) and are handed out to be written, each 0 or 1 or, with
    // finish_alive(normalise), any byte with non-zero = alive; the caller's kernels; finish_alive() -- id list, count and compact
    // copies follow the flags.  grads != nullptr: the gradient records of the dead rows become +0.  A set that begin_alive()
    // creates has its list and count (every row) queued at once: a caller that fails between the two steps leaves a context
    // whose Adam launch walks a valid list.
    hipError_t begin_alive(uint8_t** flags, uint32_t* scan_temp);
    hipError_t finish_alive(float* grads, uint32_t* scan_temp);
    hipError_t clear_alive(); // every row alive again, the buffers go (waits for the stream); nothing to do without an alive set
    uint32_t* alive_scan_work() const { return held_work_; } // n words, free between begin_alive() and finish_alive()
    // The number of alive rows: known to the host after a call that told it (alive_count_is), read back (waits) otherwise.
    hipError_t alive_count(int* out);
    void alive_count_is(int count) { alive_count_ = count; }
    // What the Adam launch about to be queued updates.  (A compact copy is ahead of the id-indexed arrays from here on.)
    AdamStep adam_step();

private:
    hipError_t flush();
    hipError_t load();
    hipError_t list_alive(float* grads, uint32_t* scan_temp); // flags -> 0 / 1, id list, count (queued)

    int n_ = 0;
    hipStream_t stream_ = nullptr;
    DevBuf<float> splats_, adams_;   // n x 9, n x 18
    DevBuf<uint8_t> dormant_, held_; // n each
    DevBuf<uint32_t> held_ids_, held_count_, held_work_; // ascending ids, their number, n words of scan workspace
    DevBuf<float> csplats_, cadams_; // capacity: every splat; allocated with the first held set
    bool compact_enabled_ = true;
    bool live_ = false;  // the compact arrays mirror the held splats
    bool dirty_ = false; // ... and are ahead of the id-indexed arrays (Adam steps since the last flush)
    Subset kind_ = Subset::None;
    int alive_count_ = -1; // -1: not known to the host
};

// The squared error of every iteration (main.cpp:796-805): the per-tile sums a backward pass leaves, and the ring of
// per-iteration totals.  Four things can add a pass's tile errors up, all in the same fixed order (sqerr_reduce,
// sqerr_sum_small), so the double does not depend on which did.
enum class SqerrBy {
    NoLoss,     // the pass started from a caller's image gradient: no squared error was formed, nothing changes here
    PassItself, // the launch wrote the total: the fused raster launch's last tile, or the reference-order chain
    NextAdam,   // the first workgroups of the next Adam launch; whoever reads or renumbers before that gets OwnKernel
    OwnKernel,  // sqerr_finalize, queued at once
    LossPass,   // a loss pass (s2d_loss.h): its finalize wrote the total of the squared-error term beside its own ring
};

class S2D_LOCAL SqerrTrace {
public:
    static constexpr int kCapacity = 1 << 16; // ring slots: iteration i lives in slot i % kCapacity
    static constexpr int kPinned = 4096;      // doubles of pinned(): s2d_step reads trace and status word in ONE round trip

    hipError_t create(int num_tiles, int n, const DeviceStatus* status, hipStream_t stream);
    double* tile_sqerr() const { return tile_sqerr_; } // [num_tiles] (+ the reduction's scratch behind them)
    // Who sums the tile errors of a backward pass.  whole_iteration: queued by s2d_forward_backward / s2d_step, which an
    // Adam step usually follows; fused_launch: ... and walked by the fused kernel (not by index ranges, nor counting).
    SqerrBy plan(bool whole_iteration, bool fused_launch) const;
    // The sum into iteration's slot as a job riding on another launch.
    SqerrJob job(int iteration) const;
    // A backward pass of `iteration` has been queued, and this is what becomes of its tile errors.
    hipError_t record(int iteration, SqerrBy by);
    SqerrJob take_for_adam(); // the job recorded as NextAdam, if one is waiting: the launch about to be queued does it
    int last_iteration() const { return last_; } // of the latest pass with a loss; -1: none yet
    // Totals of the iterations [first, first + count) -> out, queued; a waiting sum is queued before.
    hipError_t read(int first, int count, double* out);
    double* pinned() const { return pinned_; }
    // The context's iteration count is about to be set from outside: a waiting sum is queued now, its slot and the
    // iteration of its non-finite guard being those of the pass that left it.
    hipError_t settle();

private:
    int num_tiles_ = 0, adam_blocks_ = 0;
    const DeviceStatus* status_ = nullptr;
    hipStream_t stream_ = nullptr;
    DevBuf<double> tile_sqerr_, ring_;
    HostBuf<double> pinned_;
    int last_ = -1;
    bool waiting_ = false; // the sum of iteration last_ rides on the next Adam launch
};

// Per-splat density statistics (S2D_BWD_DENSITY_STATS): n x 3 floats -- sum |dL/dpos.x|, sum |dL/dpos.y|,
// sum T * alpha over the pixels of the slab and the passes since the last reset -- and the number of those passes.  Allocated
// (zeroed) by the first pass that asks, so a context that never does pays nothing.
class S2D_LOCAL DensityStats {
public:
    void create(int n, hipStream_t stream) { n_ = n, stream_ = stream; }
    // The array a statistics pass about to be queued accumulates into; counts the pass.
    hipError_t next_pass(float** out);
    hipError_t reset(); // zeros (queued), passes = 0
    int passes() const { return passes_; }
    const float* data() const { return buf_; } // null: no pass has asked yet (all zeros)
    int n() const { return n_; }

private:
    int n_ = 0, passes_ = 0;
    hipStream_t stream_ = nullptr;
    DevBuf<float> buf_;
};

} // namespace s2d
