// s2d_multi.h -- several GPUs behind ONE handle (include/splat2d.h "s2d_multi_*"; SURVEY.md section 8b/8e: "device
// list ... multi-GPU fan-out is internal").  Private to the handle's units: the types, and what the units share.
//
// A reference-side caller keeps its single-threaded frame loop (main.cpp:334) and gets N GPUs by swapping s2d_ctx for
// s2d_multi: the image is cut into N row slabs (whole 16-pixel tile rows), every device gets an ordinary context for
// its slab and one worker thread that keeps the context's calls in order; the caller's thread only hands out commands
// and adds up the slabs' squared errors.  Two ways to keep the devices consistent:
//
//  * slab ownership (default): a device holds -- projects, lists, updates -- only the splats that can reach its rows.
//    Per iteration the holders of a shared splat swap its partial gradient rows (s2d_rows_gather into a send buffer,
//    a peer-to-peer copy over xGMI queued on the RECEIVER's stream behind the sender's event, s2d_grads_combine in
//    rank order, so every holder forms the same bits); every 64 iterations the hold sets are refreshed from the
//    current parameters and the 27-float state of splats that drift into a neighbour's reach is handed over.  No
//    collective library involved: neighbours talk to neighbours, ~1 MB per neighbour and iteration (8 ranks, 4096^2 / 1 M) instead of a 36 MB all-reduce.
//  * replicated state (S2D_MULTI_REPLICATED, north_star's scheme): splats and Adam state on every device, the N x 9 fp32
//    gradient arrays summed in place by an RCCL all-reduce (ncclAllReduce on each context's own stream, between
//    s2d_forward_backward and s2d_adam_step), the identical Adam step everywhere.  RCCL is loaded with dlopen when
//    such a handle is created, so other users of the library never load it.
//
// S2D_MULTI_SHARE_GPU (rehearsal on a box with fewer GPUs than ranks): all ranks on the first listed device; the peer
// copies become plain device copies, the all-reduce is staged through pinned host memory in rank order.
//
// The units:
//   s2d_multi.hip             the extern "C" entry points, on the caller's thread
//   s2d_multi_run.hip         the command hand-out: the workers, a rank's share of a step, the caller's watchdog
//   s2d_multi_ownership.hip   slab ownership: hold sets, exchange plans, refreshes, the per-iteration exchange
//   s2d_multi_replicated.hip  replicated state: RCCL, the communicators, the host-staged all-reduce
//   s2d_multi_stop.hip        the barrier, the stop path, the bounded waits, the handle's health, the reports
//   s2d_multi_plan.h          the list arithmetic of slab ownership, host-only and pure
//
// Who writes what.  A Rank is written by its own thread while a command runs and by the caller's thread between
// commands; what peers and the watchdog read meanwhile is atomic (comm, sent_seq, progress), guarded by s2d_multi::m
// (done, rc, the command record) or read behind a rendezvous only (halo).  Of the handle itself the rank threads and
// the watchdog only raise atomics (late, comms_aborted, collective_lost, timed_out) and use the barrier; everything
// else -- health, hold_valid, hold_age, iterations, err -- belongs to the caller's thread.
#pragma once

#include "../../include/splat2d.h"
#include "../../include/splat2d_test.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // types only; the entry points are resolved at run time

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "s2d_owned.h"

namespace s2d {
namespace multi {

using s2d::DevBuf; // here: arrays that only grow (reserve), re-allocated while the rank's stream is idle
using s2d::Event;
using s2d::HostBuf;

struct S2D_LOCAL Rccl {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr; // frees a communicator whose collective can no longer complete
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

// Reusable barrier of the rank threads; abort() releases everybody for good once a rank has failed.  A wait is bounded:
// a rank that does not arrive within `timeout_ms` (it stopped answering -- stuck in a device wait, or dead) breaks the
// barrier for everybody instead of leaving the others asleep, and `timed_out` says so.
struct S2D_LOCAL Barrier {
    std::mutex m;
    std::condition_variable cv;
    int n = 1, waiting = 0, generation = 0;
    std::atomic<bool> broken{false};
    std::atomic<bool> timed_out{false};
    std::atomic<int> timeout_ms{0}; // 0: wait without bound
    uint64_t here = 0;              // bit r: rank r is waiting in the current generation
    std::atomic<uint64_t> missing{0}; // when a wait timed out: the ranks that had not arrived at that moment
    void wait(int rank);
    void abort();
    void reset();
};

enum Command { CMD_NONE = 0, CMD_STEP, CMD_HOLD, CMD_FORWARD, CMD_QUIT };
enum Scheme { SCHEME_NONE = 0, SCHEME_OWNERSHIP = 1, SCHEME_REPLICATED = 2 };
constexpr int kStopped = -1; // a rank that stopped because another one failed (never reported to the caller)

// What the caller's thread hands to the workers: written and read under s2d_multi::m (a worker takes a copy).
struct S2D_LOCAL CommandRecord {
    int cmd = CMD_NONE;
    int seq = 0;         // one more per hand-out: what a worker waits for
    int iters = 0;       // CMD_STEP: iterations of the call, ...
    uint32_t flags = 0;  // ... its S2D_STEP_* flags ...
    int first_iter = 0;  // ... and the iteration it starts at
};

// What a rank thread is doing, for the report when one stops answering (s2d_multi_last_error names it).
enum Phase { PH_IDLE = 0, PH_RASTER, PH_EXCHANGE, PH_ALLREDUCE, PH_ADAM, PH_REFRESH, PH_DRAIN, PH_HOLD, PH_FORWARD, PH_DONE };

struct S2D_LOCAL Progress {           // one per rank, written by its thread only
    std::atomic<uint64_t> ticks{0};   // bumped at every phase change: the watchdog of run_command looks for movement
    std::atomic<int> phase{PH_IDLE};
    std::atomic<int> iteration{0};
};

// Slab ownership, one rank's side (the host logic of distributed.HaloStep, here inside the library).
struct S2D_LOCAL HaloRank {
    std::vector<uint32_t> mask;           // per splat: bit q = rank q holds it; 0 = this rank does not (its copy is stale)
    std::vector<int32_t> held;            // ascending ids with mask != 0
    std::vector<int32_t> splits, offsets; // gradient rows swapped with each peer per iteration; where its segment starts
    int total = 0, n_rows = 0;
    bool any_exchange = false;            // some rank swaps something: everybody takes part in the per-iteration barrier
    DevBuf<int32_t> d_send_ids, d_rows, d_src;
    DevBuf<float> d_send[2], d_recv;      // two send buffers: a peer may still be copying iteration k while k + 1 is gathered
    DevBuf<uint32_t> d_mask;              // n words: s2d_halo_masks output / s2d_halo_commit input
    Event ev_sent[2];
    unsigned seq = 0;                     // exchanges since the hold sets were made (its parity picks the send buffer)
    // a refresh: state rows on their way to ranks that newly hold a splat
    std::vector<uint32_t> fresh;                 // masks from the current parameters (0 where not held)
    std::vector<std::vector<int32_t>> out_ids;   // [destination rank]
    std::vector<std::vector<uint32_t>> out_mask; // ... and the hold-set word the destination starts with
    std::vector<int32_t> out_off;                // first payload row of each destination
    DevBuf<int32_t> d_pay_ids, d_in_ids;
    DevBuf<float> d_pay_sp, d_pay_ad, d_in_sp, d_in_ad;
    long long handed = 0;                 // state rows sent or received so far (diagnostic)
};

// Everything one rank has (who writes it: the head of this file).
struct S2D_LOCAL Rank {
    int index = 0, device = 0;
    s2d_ctx* ctx = nullptr;
    int row_begin = 0, row_end = 0;
    HaloRank halo;
    std::atomic<ncclComm_t> comm{nullptr}; // the communicator slot: see abort_collective for who may empty it
    // Exchanges (since the hold sets were planned) whose gather and hipEventRecord this rank's thread has ISSUED.  A
    // receiver may call hipStreamWaitEvent on the event of exchange k only once it is recorded -- the one thing the rank
    // threads tell each other per iteration, pairwise and without sleeping (no barrier: the streams order the rest)
    std::atomic<unsigned> sent_seq{0};
    Progress progress;
    // The events of the bounded stream waits: [0], [1] mark every 64th iteration of a step (rank_step waits for the one
    // before last, so a wait never covers more than 128 iterations of device work and never leaves the device idle);
    // [2] is for one-off drains.
    Event ev_prog[3];
    HostBuf<float> staging;    // replicated + share-gpu: pinned copy of the rank's partial gradients; rank 0's receives the sum
    bool done = false;         // guarded by s2d_multi::m, like rc
    int rc = S2D_OK;
    std::string msg;           // failures of the handle's own HIP calls (the contexts keep theirs)
    std::vector<double> sqerr; // [iteration of the call]: partial squared errors

    hipStream_t stream() const { return (hipStream_t)s2d_stream(ctx); }
    // What the rank owns through the runtime goes on its device, with its stream idle (s2d_owned.h) and before its
    // context: the worker at CMD_QUIT, or s2d_multi_destroy itself when no worker was ever started.
    void let_go()
    {
        (void)hipSetDevice(device);
        halo = HaloRank();
        for (Event& e : ev_prog) e = Event();
        staging.release();
    }
};

// Whether the handle can go on, as the caller's thread knows it between commands (the rank threads and the watchdog
// only raise the atomics collective_lost and timed_out; this is what the caller derives from them).  Ordered: a worse
// state is never left for a better one, except NeedsState.
//   a step failed (s2d_multi_step): NeedsState -- the ranks stand at different iterations; Dead when a communicator was
//     aborted or a wait ran out on the way (the ranks no longer agree on where the run stands).
//   every rank's counters set alike (s2d_multi_init_splats, s2d_multi_set_adam): NeedsState back to Usable, nothing else.
//   the stop was not answered (the watchdog of run_command, in any command): Abandoned -- threads, contexts and device
//     memory are never freed, no destructor of s2d_multi or Rank runs.
// refuse() turns it into the status and message of a call that needs better.
enum class Health { Usable, NeedsState, Dead, Abandoned };

} // namespace multi
} // namespace s2d

struct S2D_LOCAL s2d_multi {
    int world = 0, W = 0, H = 0, n = 0;
    bool share_gpu = false;
    int scheme = s2d::multi::SCHEME_NONE;
    std::vector<s2d::multi::Rank> ranks; // sized once by s2d_multi_create (a Rank holds atomics and cannot move)
    s2d::multi::Rccl rccl;
    // slab ownership
    std::vector<int32_t> bounds;    // the world + 1 row bounds s2d_halo_masks takes
    int interval = 64;              // iterations between refreshes of the hold sets
    float margin = 0.0f;            // rows; must outlast one interval of Adam steps
    bool hold_valid = false;        // hold sets exist (otherwise every context holds, and has, everything)
    int hold_age = 0;               // iterations since they were made
    std::atomic<int> late{0};
    std::atomic<bool> comms_aborted{false};   // a stop was published during the current command: no rank starts a collective any more
    std::atomic<bool> collective_lost{false}; // some communicator really was aborted
    std::atomic<bool> timed_out{false};       // some wait ran out: the ranks no longer agree on where the run stands
    s2d::multi::Health health = s2d::multi::Health::Usable;
    // A rank that stops answering (a device wait that never ends, a thread that died) must not hang the caller: every
    // wait of one rank for another, and for its own stream, gives up after this long without progress (milliseconds;
    // S2D_MULTI_STALL_TIMEOUT_MS or s2d_multi_set_stall_timeout; 0 = wait for ever, the behaviour up to round 3)
    std::atomic<int> stall_ms{30000};
    // test hook (include/splat2d_test.h): rank `stall_rank` stops before its exchange of iteration `stall_iter`
    int stall_rank = -1, stall_iter = -1, stall_for_ms = 0;
    // command hand-out
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_cmd, cv_done;
    s2d::multi::CommandRecord command; // guarded by m
    int done_count = 0;                // guarded by m
    s2d::multi::Barrier barrier;
    double mse_norm = 1.0;          // H * W * 3, main.cpp:805
    int iterations = 0;
    char err[1280] = {0};
};

namespace s2d {
namespace multi {

#define MHIP(R, call)                                                                                 \
    do {                                                                                              \
        const hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return rank_fail((R), S2D_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// ---- s2d_multi_stop.hip
S2D_LOCAL int mfail(s2d_multi* m, int code, const char* fmt, ...);
S2D_LOCAL int rank_fail(Rank& R, int code, const char* fmt, ...);
S2D_LOCAL void worsen(s2d_multi* m, Health to);
S2D_LOCAL void state_set_afresh(s2d_multi* m);
S2D_LOCAL int refuse(s2d_multi* m, Health limit);
S2D_LOCAL const char* phase_name(int p);
S2D_LOCAL void at_phase(Rank& R, int phase, int iteration);
S2D_LOCAL void abort_collective(s2d_multi* m, Rank& Q);
S2D_LOCAL void stop_everybody(s2d_multi* m, Rank& R);
S2D_LOCAL int wait_ran_out(s2d_multi* m, Rank& R, const char* fmt, ...);
S2D_LOCAL bool stopped(s2d_multi* m, Rank& R);
S2D_LOCAL int meet_rank(s2d_multi* m, Rank& R, const char* where);
S2D_LOCAL int wait_event(s2d_multi* m, Rank& R, hipEvent_t ev, const char* what);
S2D_LOCAL int drain_now(s2d_multi* m, Rank& R, const char* what);

// "Which ranks, where", for the reports: `one(Q, text, capacity)` writes the words for rank Q; those of the ranks
// `which(Q)` picks are joined with `separator`.
template <typename Which, typename One>
std::string list_ranks(s2d_multi* m, const char* separator, Which which, One one)
{
    std::string out;
    for (Rank& Q : m->ranks)
        if (which(Q)) {
            char text[128];
            one(Q, text, sizeof(text));
            if (!out.empty()) out += separator;
            out += text;
        }
    return out;
}

// ---- s2d_multi_replicated.hip
S2D_LOCAL int set_up_replicated(s2d_multi* m); // s2d_multi_create: the communicators, or the staging buffers of a shared GPU
S2D_LOCAL void destroy_communicator(s2d_multi* m, Rank& R);
S2D_LOCAL int all_reduce_grads(s2d_multi* m, Rank& R);

// ---- s2d_multi_ownership.hip
S2D_LOCAL int set_up_peer_access(s2d_multi* m); // s2d_multi_create
S2D_LOCAL int hold_fresh(s2d_multi* m, Rank& R);
S2D_LOCAL int refresh(s2d_multi* m, Rank& R);
S2D_LOCAL int exchange_grads(s2d_multi* m, Rank& R);
S2D_LOCAL int assemble_splats(s2d_multi* m, s2d_splat* out);
S2D_LOCAL int assemble_adam(s2d_multi* m, s2d_splat_adam* out);

// ---- s2d_multi_run.hip
S2D_LOCAL void start_workers(s2d_multi* m);
S2D_LOCAL void quit_workers(s2d_multi* m);
S2D_LOCAL void run_command(s2d_multi* m, int cmd, int iters = 0, uint32_t flags = 0, int first_iter = 0);
S2D_LOCAL int first_failure(s2d_multi* m, const char* what);
S2D_LOCAL int ensure_hold(s2d_multi* m);

} // namespace multi
} // namespace s2d
