// s2d_multi_run.hip -- the command hand-out of the multi-device handle (s2d_multi.h): the caller's thread writes a
// command record, every rank's worker thread runs its share of it, the caller waits for all of them with a watchdog.
#include "s2d_multi.h"

#include <algorithm>
#include <chrono>
#include <cstdio>

namespace s2d {
namespace multi {

namespace {

// Test hook (s2d_test_multi_stall): the chosen rank's thread stops answering before its exchange of the chosen iteration.
void stall_if_asked(s2d_multi* m, const Rank& R, int iteration)
{
    if (R.index != m->stall_rank || iteration != m->stall_iter) return;
    const auto t0 = std::chrono::steady_clock::now();
    while (!m->barrier.broken && (m->stall_for_ms < 0 || std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(m->stall_for_ms)))
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
}

// No refresh paces the schemes without hold sets: rank_step marks every 64th iteration on the stream (`marks` so far
// in this call) and waits here for the mark BEFORE the one just recorded, so the host never runs more than 128
// iterations ahead of the device, the device never waits for the host, and a device that stopped is noticed within
// the stall limit.
int pace_batch(s2d_multi* m, Rank& R, int it, int marks)
{
    if (marks < 2) return S2D_OK;
    at_phase(R, PH_DRAIN, it);
    return wait_event(m, R, R.ev_prog[marks & 1], "running a batch of 64 iterations");
}

// One rank's share of s2d_multi_step: `iters` frames of main.cpp:334 on its rows.  A rank that fails before it has
// queued its share of a collective would leave the others waiting inside theirs for good: it stops everybody.
int rank_step(s2d_multi* m, Rank& R, const CommandRecord& cmd)
{
    s2d_ctx* c = R.ctx;
    const uint32_t bwd_flags = (cmd.flags & S2D_STEP_OPTIMIZE_OPACITY) ? 0u : S2D_BWD_SKIP_OPACITY_GRAD; // main.cpp:735
    int rc = S2D_OK;
    int marks = 0; // progress marks recorded so far in this call
    for (int k = 0; k < cmd.iters && rc == S2D_OK && !m->barrier.broken; k++) {
        const bool last = k + 1 == cmd.iters;
        const int it = cmd.first_iter + k;
        at_phase(R, PH_RASTER, it);
        rc = s2d_forward_backward(c, bwd_flags | (last ? 0u : S2D_FB_SKIP_IMAGE));
        if (rc != S2D_OK) break;
        stall_if_asked(m, R, it);
        // the only exchange of the iteration
        if (m->scheme == SCHEME_OWNERSHIP) {
            at_phase(R, PH_EXCHANGE, it);
            rc = exchange_grads(m, R);
        } else if (m->scheme == SCHEME_REPLICATED) {
            at_phase(R, PH_ALLREDUCE, it);
            rc = all_reduce_grads(m, R);
        }
        if (rc == S2D_OK) {
            at_phase(R, PH_ADAM, it);
            rc = s2d_adam_step(c, cmd.flags);
        }
        if (rc == S2D_OK && m->scheme == SCHEME_OWNERSHIP && (m->hold_age + k + 1) % m->interval == 0) {
            at_phase(R, PH_REFRESH, it);
            rc = refresh(m, R);
        } else if (rc == S2D_OK && m->scheme != SCHEME_OWNERSHIP && (k + 1) % 64 == 0 && !last) {
            MHIP(R, hipEventRecord(R.ev_prog[marks & 1], R.stream()));
            rc = pace_batch(m, R, it, ++marks);
        }
    }
    R.sqerr.assign((size_t)cmd.iters, 0.0);
    // A rank that failed on the way (not the finite guard below, which every replica sees alike and which leaves every
    // collective queued): the others may already sit in an all-reduce that will never get this rank's share
    if (rc != S2D_OK && rc != kStopped) stop_everybody(m, R);
    if (rc == S2D_OK) {
        at_phase(R, PH_DRAIN, cmd.first_iter + cmd.iters);
        rc = drain_now(m, R, "finishing the iterations of this call");
    }
    if (rc == S2D_OK && cmd.iters > 0) rc = s2d_get_sqerr_trace(c, cmd.first_iter, cmd.iters, R.sqerr.data());
    if (rc == S2D_OK) rc = s2d_synchronize(c); // the finite guard, main.cpp:752-785
    if (rc != S2D_OK) m->barrier.abort();      // the other ranks stop at their next wait instead of sitting in it
    return rc;
}

void worker_main(s2d_multi* m, Rank* rank)
{
    Rank& R = *rank;
    int seen = 0;
    for (;;) {
        CommandRecord cmd;
        {
            std::unique_lock<std::mutex> lk(m->m);
            m->cv_cmd.wait(lk, [&] { return m->command.seq != seen; });
            cmd = m->command;
            seen = cmd.seq;
        }
        if (cmd.cmd == CMD_QUIT) {
            R.let_go(); // here, on its device, not with the handle
            return;
        }
        int rc = S2D_OK;
        if (cmd.cmd == CMD_STEP) rc = rank_step(m, R, cmd);
        if (cmd.cmd == CMD_HOLD) {
            at_phase(R, PH_HOLD, 0);
            rc = hold_fresh(m, R);
            if (rc != S2D_OK) m->barrier.abort();
        }
        if (cmd.cmd == CMD_FORWARD) { // the rank's rows of image0 from the current parameters (it holds every splat that reaches them)
            at_phase(R, PH_FORWARD, 0);
            rc = s2d_forward(R.ctx);
            if (rc == S2D_OK) rc = drain_now(m, R, "rendering its rows");
            if (rc == S2D_OK) rc = s2d_synchronize(R.ctx);
        }
        at_phase(R, PH_DONE, 0);
        {
            std::lock_guard<std::mutex> lk(m->m);
            R.rc = rc;
            R.done = true;
            m->done_count++;
        }
        m->cv_done.notify_one();
    }
}

} // namespace

void start_workers(s2d_multi* m)
{
    for (Rank& R : m->ranks) m->workers.emplace_back(worker_main, m, &R);
}

// s2d_multi_destroy: every worker lets its rank's resources go (Rank::let_go) and ends.
void quit_workers(s2d_multi* m)
{
    if (m->workers.empty()) return;
    {
        std::lock_guard<std::mutex> lk(m->m);
        m->command.cmd = CMD_QUIT;
        m->command.seq++;
    }
    m->cv_cmd.notify_all();
    for (auto& t : m->workers) t.join();
}

// Hand `cmd` to every worker and wait for all of them -- with a watchdog: the ranks' own waits are bounded (wait_issued,
// wait_event, the barrier), but a rank can also sit inside a runtime call the handle cannot bound (a synchronous copy in
// a context's list rebuild behind a kernel that never ends, a collective's submission).  When NO rank has changed phase
// for twice the stall limit the caller stops everybody, gives the ranks one more limit to come back, and otherwise
// returns without them: the handle is then Abandoned -- its threads and contexts are never freed (a thread inside a
// runtime call cannot be cancelled) -- and every later call is refused.
void run_command(s2d_multi* m, int cmd, int iters, uint32_t flags, int first_iter)
{
    m->late = 0;
    m->comms_aborted.store(false); // (a dead handle never gets here)
    m->barrier.reset();
    m->barrier.timeout_ms = m->stall_ms.load() > 0 ? 2 * m->stall_ms.load() : 0;
    {
        std::lock_guard<std::mutex> lk(m->m);
        m->command = CommandRecord{cmd, m->command.seq + 1, iters, flags, first_iter};
        m->done_count = 0;
        for (Rank& R : m->ranks) {
            R.msg.clear();
            R.done = false;
        }
    }
    m->cv_cmd.notify_all();
    std::unique_lock<std::mutex> lk(m->m);
    const auto all_done = [&] { return m->done_count == m->world; };
    uint64_t seen = 0;
    auto moved = std::chrono::steady_clock::now();
    bool stopping = false;
    for (;;) {
        const int limit = m->stall_ms.load();
        if (limit <= 0) {
            m->cv_done.wait(lk, all_done);
            return;
        }
        if (m->cv_done.wait_for(lk, std::chrono::milliseconds(std::max(10, std::min(250, limit / 4))), all_done)) return;
        uint64_t ticks = (uint64_t)m->done_count;
        for (const Rank& R : m->ranks) ticks += R.progress.ticks.load(std::memory_order_acquire);
        const auto now = std::chrono::steady_clock::now();
        if (ticks != seen) {
            seen = ticks;
            moved = now;
            continue;
        }
        const long long quiet = std::chrono::duration_cast<std::chrono::milliseconds>(now - moved).count();
        if (!stopping && quiet > 2LL * limit + 1000) {
            stopping = true;
            moved = now;
            m->timed_out.store(true);
            m->comms_aborted.store(true);
            m->barrier.abort();
            // last resort for a rank that sits inside a collective's submission or behind its kernel and cannot look up
            // (abort_collective: the window this leaves open)
            for (Rank& R : m->ranks)
                if (!R.done) abort_collective(m, R);
        } else if (stopping && quiet > (long long)limit + 1000) {
            const std::string who = list_ranks(m, "; ", [](const Rank& R) { return !R.done; }, [](const Rank& R, char* text, size_t capacity) {
                snprintf(text, capacity, "rank %d (device %d) at '%s', iteration %d", R.index, R.device, phase_name(R.progress.phase.load()),
                         R.progress.iteration.load());
            });
            for (Rank& R : m->ranks)
                if (!R.done) R.rc = S2D_E_STATE; // (under m->m, like the workers' own writes; their message strings are theirs)
            worsen(m, Health::Abandoned);
            snprintf(m->err, sizeof(m->err), "no rank made progress for %d ms and the stop was not answered: %s; the handle is abandoned "
                                             "(its threads and device memory are not freed)", 3 * limit + 2000, who.c_str());
            return;
        }
    }
}

int first_failure(s2d_multi* m, const char* what)
{
    if (m->health == Health::Abandoned) return S2D_E_STATE; // run_command wrote the report
    for (const Rank& R : m->ranks)
        if (R.rc != S2D_OK && R.rc != kStopped)
            return mfail(m, R.rc, "%s on rank %d (device %d): %s", what, R.index, R.device, R.msg.empty() ? s2d_last_error(R.ctx) : R.msg.c_str());
    for (const Rank& R : m->ranks)
        if (R.rc != S2D_OK) return mfail(m, S2D_E_STATE, "%s: rank %d stopped without a failing rank", what, R.index);
    return S2D_OK;
}

// Slab ownership: make the hold sets if the replicas were (re)filled since the last time.
int ensure_hold(s2d_multi* m)
{
    if (m->scheme != SCHEME_OWNERSHIP || m->hold_valid) return S2D_OK;
    run_command(m, CMD_HOLD);
    if (int rc = first_failure(m, "making the hold sets")) return rc;
    m->hold_valid = true;
    m->hold_age = 0;
    return S2D_OK;
}

} // namespace multi
} // namespace s2d
