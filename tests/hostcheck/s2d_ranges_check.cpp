// s2d_ranges_check.cpp -- TEST SHIM.  Compiles the cutter of index-range rendering
// (2dgaussiansplatting_amd/csrc/s2d_ranges.h, the very function the library calls) for the host, so that
// tests/test_index_ranges_cpu.py can run it on inputs of its own.  Not a fallback: the product never links this.
#include "../../2dgaussiansplatting_amd/csrc/s2d_ranges.h"

// out: room for n + 2 entries (a cut in front of every splat but the first, and the two ends).  Returns how many were written.
extern "C" int ir_cut(const uint32_t* counts, int n, uint64_t budget, int32_t* out)
{
    const std::vector<int> r = s2d::cut_index_ranges(counts, n, budget);
    for (size_t k = 0; k < r.size(); k++) out[k] = r[k];
    return (int)r.size();
}

// The growth rule of pair-sized memory (RasterSurface::ensure_pairs) and the bound it clamps at.
extern "C" uint64_t ir_pair_capacity(uint64_t need) { return s2d::pair_capacity(need); }
extern "C" uint64_t ir_max_pairs(void) { return s2d::kMaxPairs; }
