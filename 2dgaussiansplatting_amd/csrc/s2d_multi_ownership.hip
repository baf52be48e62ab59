// s2d_multi_ownership.hip -- slab ownership of the multi-device handle (the default scheme; s2d_multi.h): a rank's hold
// set and exchange plan, the refresh that hands splats from rank to rank, the exchange of every iteration.  Which ids
// go where is decided in s2d_multi_plan.h; here are the device buffers, the copies and the rendezvous around it.
#include "s2d_multi.h"

#include <chrono>

#include "s2d_multi_plan.h"

namespace s2d {
namespace multi {

// One rank per GPU, and direct peer-to-peer copies where the fabric allows them (the copies work without, staged).
int set_up_peer_access(s2d_multi* m)
{
    for (const Rank& A : m->ranks)
        for (const Rank& B : m->ranks) {
            if (&A == &B) continue;
            if (A.device == B.device) {
                if (!m->share_gpu) return mfail(m, S2D_E_INVALID, "device %d listed twice (S2D_MULTI_SHARE_GPU rehearses several ranks on one GPU)", A.device);
                continue;
            }
            int can = 0;
            if (hipSetDevice(A.device) != hipSuccess) return mfail(m, S2D_E_HIP, "hipSetDevice(%d)", A.device);
            if (hipDeviceCanAccessPeer(&can, A.device, B.device) == hipSuccess && can) {
                const hipError_t e = hipDeviceEnablePeerAccess(B.device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError(); // copies are staged then
            }
        }
    return S2D_OK;
}

namespace {

// Device-to-device copy between two ranks' buffers, queued on `stream` (the receiver's): over xGMI between two GPUs,
// an ordinary device copy when the ranks share one.
hipError_t rank_copy(void* dst, const Rank& to, const void* src, const Rank& from, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) return hipSuccess;
    if (to.device == from.device) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream);
    return hipMemcpyPeerAsync(dst, to.device, src, from.device, bytes, stream);
}

// The hold words from the current parameters, into H.fresh.
int read_hold_words(s2d_multi* m, Rank& R)
{
    HaloRank& H = R.halo;
    if (int rc = s2d_halo_masks(R.ctx, m->world, m->bounds.data(), m->margin, H.d_mask)) return rc;
    MHIP(R, hipMemcpyAsync(H.fresh.data(), H.d_mask, (size_t)m->n * 4, hipMemcpyDeviceToHost, R.stream()));
    return drain_now(m, R, "reading the hold-set words");
}

// Exchange lists for the rank's current hold set (s2d::exchange_plan), and their copy on the device.
int plan(s2d_multi* m, Rank& R)
{
    HaloRank& H = R.halo;
    hipStream_t stream = R.stream();
    std::vector<int32_t> send_ids, rows, src;
    const int total = exchange_plan(H.mask, H.held, R.index, m->world, &send_ids, &H.splits, &H.offsets, &rows, &src);
    H.total = total;
    H.n_rows = (int)rows.size();
    H.seq = 0;
    R.sent_seq.store(0u, std::memory_order_release); // every rank thread is behind a barrier here, none is waiting on it
    MHIP(R, H.d_send_ids.reserve((size_t)total));
    MHIP(R, H.d_send[0].reserve((size_t)total * 9));
    MHIP(R, H.d_send[1].reserve((size_t)total * 9));
    MHIP(R, H.d_recv.reserve((size_t)total * 9));
    MHIP(R, H.d_rows.reserve(rows.size()));
    MHIP(R, H.d_src.reserve(src.size()));
    if (total) MHIP(R, hipMemcpyAsync(H.d_send_ids, send_ids.data(), (size_t)total * 4, hipMemcpyHostToDevice, stream));
    if (!rows.empty()) {
        MHIP(R, hipMemcpyAsync(H.d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, stream));
        MHIP(R, hipMemcpyAsync(H.d_src, src.data(), src.size() * 4, hipMemcpyHostToDevice, stream));
    }
    return drain_now(m, R, "uploading its exchange plan"); // the host vectors go away
}

// After the plans of all ranks are in (behind a barrier): does anybody swap anything, and do the two sides of every
// pair agree on how much?
int settle_plans(s2d_multi* m, Rank& R)
{
    HaloRank& H = R.halo;
    H.any_exchange = false;
    for (const Rank& P : m->ranks) {
        H.any_exchange = H.any_exchange || P.halo.total > 0;
        const int mine = H.splits[(size_t)P.index], theirs = P.halo.splits[(size_t)R.index];
        if (&P != &R && theirs != mine)
            return rank_fail(R, S2D_E_STATE, "slab ownership: ranks %d and %d disagree on the rows they share (%d vs %d)", R.index, P.index, mine, theirs);
    }
    return S2D_OK;
}

// The end of hold_fresh and of refresh: the rank's new hold-set words (H.mask) go to its context -- `arrivals`: some
// splat is new here, the tile lists are stale -- its exchange plan is made, and behind the rendezvous `where` the
// plans of all ranks are checked against each other.
int adopt_hold_set(s2d_multi* m, Rank& R, bool arrivals, const char* where)
{
    HaloRank& H = R.halo;
    MHIP(R, hipMemcpyAsync(H.d_mask, H.mask.data(), (size_t)m->n * 4, hipMemcpyHostToDevice, R.stream()));
    if (int rc = s2d_halo_commit(R.ctx, H.d_mask, R.index, arrivals)) return rc;
    if (int rc = plan(m, R)) return rc;
    if (int rc = meet_rank(m, R, where)) return rc; // plans are in; after a refresh the outgoing buffers may be re-used
    return settle_plans(m, R);
}

// A refresh, phase "send": the state rows this rank hands over (H.out_ids, one segment per destination) are gathered
// into its payload buffers, where the destinations fetch them.  Returns their number in *k_out.
int gather_outgoing(s2d_multi* m, Rank& R, int* k_out)
{
    HaloRank& H = R.halo;
    std::vector<int32_t> pay_ids;
    for (const Rank& Q : m->ranks) {
        const std::vector<int32_t>& ids = H.out_ids[(size_t)Q.index];
        H.out_off[(size_t)Q.index] = (int32_t)pay_ids.size();
        pay_ids.insert(pay_ids.end(), ids.begin(), ids.end());
    }
    const int k = *k_out = (int)pay_ids.size();
    if (!k) return S2D_OK;
    MHIP(R, H.d_pay_ids.reserve((size_t)k));
    MHIP(R, H.d_pay_sp.reserve((size_t)k * 9));
    MHIP(R, H.d_pay_ad.reserve((size_t)k * 18));
    MHIP(R, hipMemcpyAsync(H.d_pay_ids, pay_ids.data(), (size_t)k * 4, hipMemcpyHostToDevice, R.stream()));
    if (int rc = s2d_rows_gather(R.ctx, S2D_ROWS_SPLATS, H.d_pay_ids, k, H.d_pay_sp)) return rc;
    if (int rc = s2d_rows_gather(R.ctx, S2D_ROWS_ADAM, H.d_pay_ids, k, H.d_pay_ad)) return rc;
    return drain_now(m, R, "gathering the state rows it hands over");
}

// A refresh, phase "receive": the state rows handed to this rank, in sender order, copied out of the senders' payload
// buffers (every rank's are in place, every stream is idle).  *late: how many arrive already touching this rank's rows.
int fetch_incoming(s2d_multi* m, Rank& R, std::vector<int32_t>* in_ids, std::vector<uint32_t>* in_mask, int* late)
{
    HaloRank& H = R.halo;
    hipStream_t stream = R.stream();
    const int r = R.index;
    for (const Rank& P : m->ranks)
        if (&P != &R) {
            in_ids->insert(in_ids->end(), P.halo.out_ids[(size_t)r].begin(), P.halo.out_ids[(size_t)r].end());
            in_mask->insert(in_mask->end(), P.halo.out_mask[(size_t)r].begin(), P.halo.out_mask[(size_t)r].end());
        }
    const int k_in = (int)in_ids->size();
    *late = 0;
    if (!k_in) return S2D_OK;
    MHIP(R, H.d_in_ids.reserve((size_t)k_in));
    MHIP(R, H.d_in_sp.reserve((size_t)k_in * 9));
    MHIP(R, H.d_in_ad.reserve((size_t)k_in * 18));
    MHIP(R, hipMemcpyAsync(H.d_in_ids, in_ids->data(), (size_t)k_in * 4, hipMemcpyHostToDevice, stream));
    size_t off = 0;
    for (const Rank& P : m->ranks)
        if (&P != &R) {
            const size_t cnt = P.halo.out_ids[(size_t)r].size(), from = (size_t)P.halo.out_off[(size_t)r];
            if (!cnt) continue;
            MHIP(R, rank_copy(H.d_in_sp + off * 9, R, P.halo.d_pay_sp + from * 9, P, cnt * 9 * sizeof(float), stream));
            MHIP(R, rank_copy(H.d_in_ad + off * 18, R, P.halo.d_pay_ad + from * 18, P, cnt * 18 * sizeof(float), stream));
            off += cnt;
        }
    std::vector<float> sp((size_t)k_in * 9);
    MHIP(R, hipMemcpyAsync(sp.data(), H.d_in_sp, sp.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (int rc = drain_now(m, R, "fetching the state rows handed to it")) return rc;
    // a splat that arrives already touching this rank's rows was rasterised here without being listed: the margin
    // did not outlast the interval
    *late = late_arrivals(sp.data(), k_in, R.row_begin, R.row_end);
    return S2D_OK;
}

// Has rank P's thread issued (gathered + recorded the event of) exchange number `seq`?  Spins without sleeping at first:
// the threads queue an iteration in tens of microseconds and run at the same pace, so the wait is short.  A failed rank
// ends it (kStopped); a rank that does not answer within the stall limit ends it too, with a report that names it
// (S2D_E_STATE): the reference's only failure policy is abort() (main.cpp:752-785), the boundary turns "a rank stopped
// answering" into a status like the rest.
int wait_issued(s2d_multi* m, Rank& R, const Rank& P, unsigned seq)
{
    const int limit = m->stall_ms.load();
    std::chrono::steady_clock::time_point t0;
    for (unsigned spins = 0; P.sent_seq.load(std::memory_order_acquire) < seq; spins++) {
        if (stopped(m, R)) return kStopped;
        if (spins <= 64) continue;
        if (spins == 65) t0 = std::chrono::steady_clock::now();
        if (spins < 4096) {
            std::this_thread::yield();
            continue;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (limit > 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(limit))
            return wait_ran_out(m, R, "rank %d (device %d) stopped answering: it has not issued gradient exchange %u (iteration %d) "
                                      "%d ms after rank %d asked for it; it was last seen at '%s', iteration %d", P.index, P.device, seq,
                                R.progress.iteration.load(), limit, R.index, phase_name(P.progress.phase.load()), P.progress.iteration.load());
    }
    return S2D_OK;
}

// Slab ownership: the complete parameter or Adam array, every row from its lowest-ranked holder.
template <typename Row, typename Get>
int assemble(s2d_multi* m, Row* out, Get get)
{
    std::vector<Row> tmp((size_t)m->n);
    for (const Rank& R : m->ranks) {
        if (int rc = get(R.ctx, tmp.data())) return mfail(m, rc, "reading rank %d: %s", R.index, s2d_last_error(R.ctx));
        for (const int32_t i : R.halo.held)
            if (lowest_holder(R.halo.mask[(size_t)i], R.index)) out[(size_t)i] = tmp[(size_t)i];
    }
    return S2D_OK;
}

} // namespace

// Hold sets from scratch; every context holds a complete, identical copy of the splats and the Adam state.
int hold_fresh(s2d_multi* m, Rank& R)
{
    HaloRank& H = R.halo;
    const int r = R.index;
    const size_t n = (size_t)m->n, world = (size_t)m->world;
    MHIP(R, hipSetDevice(R.device));
    for (Event& e : H.ev_sent)
        if (!e) MHIP(R, e.create(hipEventDisableTiming));
    if (int rc = s2d_halo_commit(R.ctx, nullptr, r, 0)) return rc; // hold everything: the masks below cover every splat
    MHIP(R, H.d_mask.reserve(n));
    H.fresh.resize(n);
    H.mask.assign(n, 0u);
    H.held.clear();
    H.out_ids.assign(world, {});
    H.out_mask.assign(world, {});
    H.out_off.assign(world, 0);
    if (int rc = read_hold_words(m, R)) return rc;
    for (size_t i = 0; i < n; i++)
        if ((H.fresh[i] >> r) & 1u) {
            H.mask[i] = H.fresh[i];
            H.held.push_back((int32_t)i);
        }
    return adopt_hold_set(m, R, true, "hold sets");
}

// Refresh the hold sets from the current parameters (every `interval` iterations).  A splat that has come within
// reach + margin of a rank that does not hold it yet is handed over -- parameters and Adam moments, by its
// lowest-ranked holder -- before it can touch that rank's rows; a holder it has left drops it.
int refresh(s2d_multi* m, Rank& R)
{
    HaloRank& H = R.halo;
    s2d_ctx* c = R.ctx;
    // masks
    if (int rc = drain_now(m, R, "finishing the iterations before a hold-set refresh")) return rc; // up to `interval` iterations of device work
    if (int rc = s2d_synchronize(c)) return rc; // the finite guard; and every copy this rank queued has landed
    if (int rc = read_hold_words(m, R)) return rc;
    // decide
    std::vector<int32_t> keep;
    decide_handover(&H.mask, H.fresh, H.held, R.index, &keep, &H.out_ids, &H.out_mask);
    // send: outgoing state rows, one segment per destination
    int k_out = 0;
    if (int rc = gather_outgoing(m, R, &k_out)) return rc;
    if (int rc = meet_rank(m, R, "hold-set refresh (state rows out)")) return rc; // every rank's outgoing rows are in place, every stream is idle
    // receive and check: incoming state rows, in sender order
    std::vector<int32_t> in_ids;
    std::vector<uint32_t> in_mask;
    int late = 0;
    if (int rc = fetch_incoming(m, R, &in_ids, &in_mask, &late)) return rc;
    const int k_in = (int)in_ids.size();
    if (late) m->late.fetch_add(late);
    if (int rc = meet_rank(m, R, "hold-set refresh (state rows in)")) return rc; // everybody has fetched its rows and reported late arrivals
    if (m->late.load() > 0)        // fatal on every rank alike
        return rank_fail(R, S2D_E_STATE, "slab ownership: %d splat(s) reached the rows of a rank before their state was handed "
                                         "over (%d on rank %d): the margin of %.1f rows did not outlast %d iterations",
                         m->late.load(), late, R.index, (double)m->margin, m->interval);
    // adopt
    if (k_in) {
        if (int rc = s2d_rows_scatter(c, S2D_ROWS_SPLATS, H.d_in_ids, k_in, H.d_in_sp)) return rc;
        if (int rc = s2d_rows_scatter(c, S2D_ROWS_ADAM, H.d_in_ids, k_in, H.d_in_ad)) return rc;
    }
    merge_arrivals(in_ids, in_mask, &H.mask, &keep);
    H.held.swap(keep);
    H.handed += k_out + k_in;
    return adopt_hold_set(m, R, k_in > 0, "hold-set refresh (plans)"); // departures alone leave the tile lists valid
}

// The iteration's exchange: the partial gradient rows of splats this rank shares go to their other holders, theirs
// come here, and every holder adds the partials in rank order.  Stream-ordered: the rank gathers its rows into one of
// two send buffers and records an event; on its OWN stream it waits for each neighbour's event of the same exchange and
// copies its segment out of the neighbour's buffer.  The rank threads do not meet: a receiver only makes sure, pairwise,
// that the sender's thread has already recorded that event (sent_seq) -- all `iters` iterations of a call are queued
// without a barrier, the refreshes stay the only rendezvous.  Buffer b of exchange k is gathered again at k + 2: by then
// this rank's stream has waited for every neighbour's event k + 1, which that neighbour recorded behind its copy of k
// (exchanges are symmetric: who receives from a rank also sends to it), and the neighbour's thread called
// hipStreamWaitEvent for k before it recorded k + 1, so re-recording the event at k + 2 cannot overtake that call.
int exchange_grads(s2d_multi* m, Rank& R)
{
    HaloRank& H = R.halo;
    if (!H.any_exchange) return S2D_OK;
    s2d_ctx* c = R.ctx;
    hipStream_t stream = R.stream();
    const unsigned seq = ++H.seq;
    const int b = (int)((seq - 1u) & 1u);
    if (H.total) {
        if (int rc = s2d_rows_gather(c, S2D_ROWS_GRADS, H.d_send_ids, H.total, H.d_send[b])) return rc;
        MHIP(R, hipEventRecord(H.ev_sent[b], stream));
    }
    R.sent_seq.store(seq, std::memory_order_release);
    for (const Rank& P : m->ranks) {
        const int cnt = H.splits[(size_t)P.index];
        if (&P == &R || cnt == 0) continue;
        if (int rc = wait_issued(m, R, P, seq)) return rc;
        MHIP(R, hipStreamWaitEvent(stream, P.halo.ev_sent[b], 0));
        MHIP(R, rank_copy(H.d_recv + (size_t)H.offsets[(size_t)P.index] * 9, R, P.halo.d_send[b] + (size_t)P.halo.offsets[(size_t)R.index] * 9, P,
                          (size_t)cnt * 9 * sizeof(float), stream));
    }
    if (H.n_rows)
        if (int rc = s2d_grads_combine(c, H.d_rows, H.n_rows, H.d_src, m->world, H.d_recv)) return rc;
    return S2D_OK;
}

int assemble_splats(s2d_multi* m, s2d_splat* out)
{
    return assemble(m, out, [](s2d_ctx* c, s2d_splat* p) { return s2d_get_splats(c, p); });
}

int assemble_adam(s2d_multi* m, s2d_splat_adam* out)
{
    return assemble(m, out, [](s2d_ctx* c, s2d_splat_adam* p) { return s2d_get_adam(c, p, nullptr, nullptr, nullptr); });
}

} // namespace multi
} // namespace s2d
