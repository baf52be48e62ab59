// s2d_multi_plan.h -- the list arithmetic of slab ownership (s2d_multi_ownership.hip): which rows a rank owns, which
// gradient rows it swaps with which peer, who hands which splat to whom at a refresh, which arrivals come too late.
// Pure functions of their arguments: no HIP, no handle, no thread; compiled by hipcc into the library and by g++ into
// the tests' shim (tests/hostcheck/s2d_multi_plan_check.cpp), which holds them to distributed.HaloStep and
// distributed.slab_rows (tests/test_multi_plan_cpu.py).  The outputs are records the rank keeps: they are cleared and
// filled, never replaced.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace s2d {

// Rows [r0, r1) of rank `rank`: whole 16-pixel tile rows, as even as possible (== distributed.slab_rows).
static inline void slab_rows(int height, int rank, int world, int* r0, int* r1)
{
    const int tile_rows = (height + 15) / 16;
    *r0 = (int)((long long)tile_rows * rank / world) * 16;
    *r1 = (int)((long long)tile_rows * (rank + 1) / world) * 16;
    if (*r1 > height) *r1 = height;
}

static inline bool lowest_holder(uint32_t mask, int r) { return mask != 0u && (mask & (0u - mask)) == (1u << r); }

// Exchange lists for a rank's hold set (`mask`: its hold words, 0 where it does not hold; `held`: the ascending ids
// with mask != 0): which gradient rows go to which peer (`send_ids`: one segment per peer, `splits[p]` ids from
// `offsets[p]` on, ascending -- the peer derives the same list from its identical mask words), and for every shared
// row (`rows`) where each holder's partial sits in the receive buffer (`src`, rows x world: s2d_grads_combine's table;
// -2 this rank's own partial, -1 not a holder).  Returns the number of rows swapped per iteration, all peers together.
static inline int exchange_plan(const std::vector<uint32_t>& mask, const std::vector<int32_t>& held, int rank, int world_,
                                std::vector<int32_t>* send_ids, std::vector<int32_t>* splits, std::vector<int32_t>* offsets,
                                std::vector<int32_t>* rows_, std::vector<int32_t>* src_)
{
    const size_t world = (size_t)world_, r = (size_t)rank;
    const uint32_t me = 1u << rank;
    std::vector<std::vector<int32_t>> peer(world);
    std::vector<int32_t>&rows = *rows_, &src = *src_;
    rows.clear();
    src.clear();
    for (const int32_t i : held) {
        uint32_t others = mask[(size_t)i] & ~me;
        if (!others) continue;
        const size_t u = rows.size();
        rows.push_back(i);
        src.resize((u + 1) * world, -1);
        src[u * world + r] = -2;
        while (others) {
            const size_t p = (size_t)__builtin_ctz(others);
            others &= others - 1u;
            src[u * world + p] = (int32_t)peer[p].size(); // + the peer's offset, below
            peer[p].push_back(i);
        }
    }
    splits->assign(world, 0);
    offsets->assign(world, 0);
    int total = 0;
    for (size_t p = 0; p < world; p++) {
        (*offsets)[p] = total;
        (*splits)[p] = (int32_t)peer[p].size();
        total += (*splits)[p];
    }
    for (size_t u = 0; u < rows.size(); u++)
        for (size_t p = 0; p < world; p++)
            if (src[u * world + p] >= 0) src[u * world + p] += (*offsets)[p];
    send_ids->clear();
    send_ids->reserve((size_t)total);
    for (size_t p = 0; p < world; p++) send_ids->insert(send_ids->end(), peer[p].begin(), peer[p].end());
    return total;
}

// A refresh, the decision: `fresh` holds the hold words from the current parameters.  The lowest-ranked old holder of
// a splat hands it to its new holders (`out_ids[q]`, ascending, and `out_mask[q]`: the word rank q starts with); a
// rank the splat still reaches keeps it under the new word (`keep`, ascending), a holder it has left drops it
// (mask = 0).  out_ids and out_mask have one list per rank.
static inline void decide_handover(std::vector<uint32_t>* mask, const std::vector<uint32_t>& fresh, const std::vector<int32_t>& held, int rank,
                                   std::vector<int32_t>* keep, std::vector<std::vector<int32_t>>* out_ids,
                                   std::vector<std::vector<uint32_t>>* out_mask)
{
    const uint32_t me = 1u << rank;
    for (auto& ids : *out_ids) ids.clear();
    for (auto& words : *out_mask) words.clear();
    keep->clear();
    keep->reserve(held.size());
    for (const int32_t i : held) {
        const uint32_t old = (*mask)[(size_t)i], now = fresh[(size_t)i];
        if (lowest_holder(old, rank)) { // the lowest-ranked old holder hands the splat to its new holders
            uint32_t arriving = now & ~old;
            while (arriving) {
                const int q = __builtin_ctz(arriving);
                arriving &= arriving - 1u;
                (*out_ids)[(size_t)q].push_back(i);
                (*out_mask)[(size_t)q].push_back(now);
            }
        }
        if (now & me) {
            (*mask)[(size_t)i] = now;
            keep->push_back(i);
        } else {
            (*mask)[(size_t)i] = 0u;
        }
    }
}

// A refresh, the adoption: the splats handed to this rank (`in_ids`, in sender order, with the words they start with)
// join what it kept; `held` is ascending again afterwards.
static inline void merge_arrivals(const std::vector<int32_t>& in_ids, const std::vector<uint32_t>& in_mask, std::vector<uint32_t>* mask,
                                  std::vector<int32_t>* held)
{
    if (in_ids.empty()) return;
    for (size_t j = 0; j < in_ids.size(); j++) (*mask)[(size_t)in_ids[j]] = in_mask[j];
    held->insert(held->end(), in_ids.begin(), in_ids.end());
    std::sort(held->begin(), held->end());
}

// How many of the `k` state rows (9 floats each: pos.x, pos.y, sx, sy, ...) handed to the rank of rows
// [row_begin, row_end) already touch those rows: such a splat was rasterised there without being listed.
static inline int late_arrivals(const float* sp, int k, int row_begin, int row_end)
{
    const float r0 = (float)row_begin, r1 = (float)row_end;
    int late = 0;
    for (int j = 0; j < k; j++) {
        const float* q = sp + (size_t)j * 9;
        const float reach = 3.0f * std::max(q[2], q[3]) + 2.0f;
        if (q[1] + reach >= r0 && q[1] - reach <= r1) late++;
    }
    return late;
}

} // namespace s2d
