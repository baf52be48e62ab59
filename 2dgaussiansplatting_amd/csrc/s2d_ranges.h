// s2d_ranges.h -- where index-range rendering (IndexRanges, s2d_context.h) cuts the splats, and how many (tile, splat) pairs
// the buffers of a raster surface get room for.  Pure functions of their arguments: no HIP, no state; compiled by hipcc
// into the library and by g++ into the tests' shim, like s2d_density.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace s2d {

// What 32-bit list positions address: a set of lists holds fewer pairs than this, and no buffer has room for more.
constexpr uint64_t kMaxPairs = 0xFFFF0000ull;

// Room to allocate when `need` pairs no longer fit: a quarter to spare (growing waits for the stream), 2^16 at least, kMaxPairs at most.
static inline uint64_t pair_capacity(uint64_t need)
{
    const uint64_t cap = need + need / 4 + 4096;
    return cap < (1u << 16) ? (1u << 16) : cap > kMaxPairs ? kMaxPairs : cap;
}

// counts[i]: the (tile, splat) pairs of splat i.  Returns r with r[0] = 0 and r.back() = n: range k holds the splats
// [r[k], r[k+1]), cut in front of the splat with which the running pair count would pass `budget`.  A range is never
// empty of splats (n > 0), so a single splat beyond the budget gets a range of its own; no other range exceeds it.
static inline std::vector<int> cut_index_ranges(const uint32_t* counts, int n, uint64_t budget)
{
    std::vector<int> r(1, 0);
    uint64_t acc = 0;
    for (int i = 0; i < n; i++) {
        if (acc > 0 && acc + counts[(size_t)i] > budget) {
            r.push_back(i);
            acc = 0;
        }
        acc += counts[(size_t)i];
    }
    r.push_back(n);
    return r;
}

} // namespace s2d
