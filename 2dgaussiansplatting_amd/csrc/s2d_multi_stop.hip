// s2d_multi_stop.hip -- how a command of the multi-device handle ends early, and what is said about it: the breakable
// barrier of the rank threads, the stop path, the bounded waits for a stream, the handle's health, the reports that
// name a rank which stopped answering (s2d_multi.h: the handle and its units).
#include "s2d_multi.h"

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>

namespace s2d {
namespace multi {

void Barrier::wait(int rank)
{
    std::unique_lock<std::mutex> lk(m);
    if (broken) return;
    const int gen = generation;
    here |= 1ull << (rank & 63);
    if (++waiting == n) {
        waiting = 0;
        here = 0;
        generation++;
        cv.notify_all();
        return;
    }
    const auto ready = [&] { return gen != generation || broken; };
    const int ms = timeout_ms.load();
    if (ms <= 0) {
        cv.wait(lk, ready);
    } else if (!cv.wait_for(lk, std::chrono::milliseconds(ms), ready)) {
        missing = ~here & ((n >= 64) ? ~0ull : ((1ull << n) - 1ull)); // who is not here NOW (they may show up a moment later)
        timed_out = true;
        broken = true;
        cv.notify_all();
    }
}

void Barrier::abort()
{
    std::lock_guard<std::mutex> lk(m);
    broken = true;
    cv.notify_all();
}

void Barrier::reset()
{
    std::lock_guard<std::mutex> lk(m);
    broken = false;
    timed_out = false;
    waiting = 0;
    here = 0;
    missing = 0;
}

int mfail(s2d_multi* m, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m->err, sizeof(m->err), fmt, ap);
    va_end(ap);
    return code;
}

int rank_fail(Rank& R, int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    R.msg = buf;
    return code;
}

void worsen(s2d_multi* m, Health to) { m->health = std::max(m->health, to); }
void state_set_afresh(s2d_multi* m) { if (m->health == Health::NeedsState) m->health = Health::Usable; }

// The answer to a call that needs the handle no worse than `limit`.
int refuse(s2d_multi* m, Health limit)
{
    if (m->health <= limit) return S2D_OK;
    if (m->health == Health::Abandoned) return S2D_E_STATE; // keeps the watchdog's report
    if (m->health == Health::Dead)
        return mfail(m, S2D_E_STATE, "%s; s2d_multi_destroy this handle and create a new one",
                     m->collective_lost.load() ? "a collective of this handle was aborted after a rank failed: its communicators are gone"
                                               : "a rank of this handle stopped answering and the ranks no longer agree on where the run stands");
    return mfail(m, S2D_E_STATE, "the last s2d_multi_step failed and left the ranks at different iterations: s2d_multi_init_splats, or "
                                 "s2d_multi_set_splats + s2d_multi_set_adam, first");
}

const char* phase_name(int p)
{
    static const char* const names[] = {"idle", "raster launch", "gradient exchange", "all-reduce", "Adam step", "hold-set refresh",
                                        "waiting for its stream", "making the hold sets", "forward", "done"};
    return p >= 0 && p <= PH_DONE ? names[p] : "?";
}

void at_phase(Rank& R, int phase, int iteration)
{
    R.progress.phase.store(phase, std::memory_order_relaxed);
    R.progress.iteration.store(iteration, std::memory_order_relaxed);
    R.progress.ticks.fetch_add(1, std::memory_order_release);
}

namespace {

// Where every rank's thread was last seen, for the reports below; and the rank furthest behind -- when a wait runs out
// because of a rank that stopped answering, that is the one (the waiting ranks are iterations ahead of it, or at the same
// iteration in a later phase).
std::string phase_table(s2d_multi* m)
{
    const Rank* worst = &m->ranks[0];
    long long worst_key = -1;
    const std::string out = list_ranks(m, "; ", [](const Rank&) { return true; }, [&](const Rank& Q, char* text, size_t capacity) {
        const int ph = Q.progress.phase.load(), it = Q.progress.iteration.load();
        snprintf(text, capacity, "rank %d: %s, iteration %d", Q.index, phase_name(ph), it);
        const long long key = ph == PH_DONE ? (1LL << 60) : (long long)it * 16 + ph;
        if (worst_key < 0 || key < worst_key) {
            worst_key = key;
            worst = &Q;
        }
    });
    char tail[64];
    snprintf(tail, sizeof(tail), "; furthest behind: rank %d (device %d)", worst->index, worst->device);
    return out + tail;
}

} // namespace

// Slot Q's communicator, taken out and aborted (RCCL then ends the kernels of that rank that wait for a peer which will
// never arrive): by the rank itself, or by the watchdog for a rank that cannot look up.  Only whoever empties a slot
// (exchange(nullptr): here, or destroy_communicator) frees what it held, so exactly one thread ever frees a
// communicator.  A rank submits to its OWN slot's value only, and when it empties the slot itself nothing is in
// flight.  One window remains: the watchdog of run_command aborts the communicator of a rank that does not answer,
// and that rank may be inside a collective's submission (all_reduce_grads) with the value it loaded a moment earlier
// -- an abort concurrent with a submission on the same communicator.  Nothing closes that window here; it is open
// only on the last-resort path, after every rank has been quiet for twice the stall limit.  collective_lost is set
// exactly when a slot was emptied here.  (Only a replicated handle on several GPUs has communicators; elsewhere the
// slots are empty.)
void abort_collective(s2d_multi* m, Rank& Q)
{
    const ncclComm_t c = Q.comm.exchange(nullptr);
    if (!c) return;
    m->collective_lost.store(true);
    if (m->rccl.CommAbort) (void)m->rccl.CommAbort(c);
}

// A rank has failed (or stopped answering): publish the stop FIRST -- no rank may start another collective, every rank
// thread leaves its waits -- and only then give up this rank's own communicator.  The other ranks abort theirs when they
// notice (stopped(), all_reduce_grads): a communicator is never freed under the thread that may be submitting to it.
// With a communicator gone the handle is dead afterwards: s2d_multi_destroy and a new s2d_multi_create bring it back.
void stop_everybody(s2d_multi* m, Rank& R)
{
    m->comms_aborted.store(true);
    m->barrier.abort();
    abort_collective(m, R);
}

// A wait of rank R ran out -- for a peer, a rendezvous or its own stream: the ranks no longer agree on where the run
// stands.  Says so, stops everybody and files R's report (S2D_E_STATE).
int wait_ran_out(s2d_multi* m, Rank& R, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    m->timed_out.store(true);
    stop_everybody(m, R);
    R.msg = buf;
    return S2D_E_STATE;
}

// Called by a rank thread inside its waits: has somebody stopped the command?  If collectives were declared lost
// (stop_everybody: a rank failed on the way or stopped answering) this rank gives up its communicator too.  A broken
// barrier alone does not mean that: the finite guard (main.cpp:752-785) breaks it at the END of a rank's share, with every
// collective of the call queued by everybody, and the handle stays usable.
bool stopped(s2d_multi* m, Rank& R)
{
    if (!m->barrier.broken.load(std::memory_order_acquire)) return false;
    if (m->comms_aborted.load()) abort_collective(m, R);
    return true;
}

// The rendezvous of the rank threads, for a rank: S2D_OK, kStopped (somebody else failed), or S2D_E_STATE when the wait itself ran out -- some rank
// never arrived; the first rank to notice reports it.
int meet_rank(s2d_multi* m, Rank& R, const char* where)
{
    m->barrier.wait(R.index);
    if (!m->barrier.broken) return S2D_OK;
    if (m->barrier.timed_out.exchange(false)) {
        const std::string table = phase_table(m);
        const uint64_t missing = m->barrier.missing.load();
        const std::string who = list_ranks(m, ", ", [&](const Rank& Q) { return ((missing >> Q.index) & 1ull) != 0; },
                                           [](const Rank& Q, char* text, size_t capacity) { snprintf(text, capacity, "rank %d (device %d)", Q.index, Q.device); });
        return wait_ran_out(m, R, "%s did not reach the rendezvous of the %s within %d ms (the ranks now: %s)", who.c_str(), where,
                            m->barrier.timeout_ms.load(), table.c_str());
    }
    (void)stopped(m, R);
    return kStopped;
}

// Wait, with a bound, until event `ev` (recorded on rank R's stream) has completed.  hipStreamSynchronize would wait for
// ever behind a kernel that never ends (a collective whose peer is gone, a device that stopped); an event and a poll
// let the thread notice a stop published by another rank, abort its own collective, and give up with a report.
int wait_event(s2d_multi* m, Rank& R, hipEvent_t ev, const char* what)
{
    const int limit = m->stall_ms.load();
    const auto t0 = std::chrono::steady_clock::now();
    bool aborted = false;
    for (unsigned spins = 0;; spins++) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return aborted ? kStopped : S2D_OK;
        if (e != hipErrorNotReady) return rank_fail(R, S2D_E_HIP, "hipEventQuery while %s: %s", what, hipGetErrorString(e));
        if (!aborted && stopped(m, R)) aborted = true; // keep polling: with its collective aborted the stream drains
        const long long waited = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        if (limit > 0 && waited > (aborted ? 2LL * limit : (long long)limit)) {
            if (aborted) return kStopped; // somebody else already reports; this stream is left as it is
            return wait_ran_out(m, R, "rank %d (device %d): the device did not finish the work queued on its stream within %d ms "
                                      "while %s (iteration %d) -- its own kernels, or a collective / peer wait for a rank that "
                                      "stopped answering (%s)", R.index, R.device, limit, what, R.progress.iteration.load(), phase_table(m).c_str());
        }
        if (spins < 2000) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(spins < 20000 ? 20 : 200));
    }
}

// A bounded wait for everything queued on the rank's stream so far.
int drain_now(s2d_multi* m, Rank& R, const char* what)
{
    MHIP(R, hipEventRecord(R.ev_prog[2], R.stream()));
    return wait_event(m, R, R.ev_prog[2], what);
}

} // namespace multi
} // namespace s2d
