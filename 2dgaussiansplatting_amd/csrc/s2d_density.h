// s2d_density.h -- the relocation planner of s2d_relocate: which splats move where, decided on the
// host from the density statistics.  A pure function of its arguments: no HIP, no random numbers, no state; compiled by
// hipcc into the library and by g++ into the tests' shim (with -ffp-contract=off in both, like everything that shares
// s2d_math.h), so a test can hold the library's result to this function's, bit for bit.
//
// Rules (n splats, statistics summed over `passes` passes):
//   1. w = weight / passes and a = hypot(abs_dpos) / passes, in double.
//   2. STARVED: w < min_weight; ordered by (w ascending, index ascending), the first max_moves are kept.
//   3. DONORS: the splats that are not starved (kept or not) and have a > 0; ordered by (a descending, index ascending); as
//      many as there are kept starved splats are taken, and surplus starved splats are dropped from the end.
//   4. The j-th donor is split onto the j-th starved splat.  sigma = the donor's larger scale (sx on a tie) divided by
//      `shrink`, clamped to [1, 1024] (main.cpp:744-745); u = (cos rot, sin rot) when that scale is sx, (-sin rot, cos rot)
//      otherwise (the axes of main.cpp:212-213, through sincos_f32).  The donor's row keeps everything but that scale, now
//      sigma, and its position, now pos - (0.5 sigma) u; the starved row becomes a copy of it at pos + (0.5 sigma) u -- the
//      two halves sit one NEW sigma apart.  Both positions are clamped like main.cpp:741-742.  The Adam moments of both
//      rows become zero.  Every other row is left alone.
// The starved row keeps its INDEX, and the index is the place in the blend order (main.cpp:419): the copy is blended where
// the starved splat was, not next to its donor.
// NaN statistics make a splat neither starved (w < min_weight is false) nor a donor (a > 0 is false).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "s2d_math.h"

namespace s2d {

// splats: n x 9 (s2d_splat), adams: n x 18 (s2d_splat_adam), stats: n x 3 (s2d_density); splats and adams are changed in
// place.  changed_ids (room for 2 * min(max_moves, n) entries): donor 0, starved 0, donor 1, starved 1, ...
// Returns the number of moves (pairs).
static inline int density_plan(int n, const float* stats, int passes, int max_moves, float min_weight, float shrink, int W, int H,
                               float* splats, float* adams, int32_t* changed_ids)
{
    if (n <= 0 || passes <= 0 || max_moves <= 0) return 0;
    struct Key {
        double v;
        int i;
    };
    std::vector<Key> starved, donors;
    for (int i = 0; i < n; i++) {
        const double w = (double)stats[3 * (size_t)i + 2] / (double)passes;
        const double a = ::hypot((double)stats[3 * (size_t)i], (double)stats[3 * (size_t)i + 1]) / (double)passes;
        if (w < (double)min_weight) starved.push_back(Key{w, i});
        else if (a > 0.0) donors.push_back(Key{a, i});
    }
    std::sort(starved.begin(), starved.end(), [](const Key& x, const Key& y) { return x.v < y.v || (x.v == y.v && x.i < y.i); });
    std::sort(donors.begin(), donors.end(), [](const Key& x, const Key& y) { return x.v > y.v || (x.v == y.v && x.i < y.i); });
    const size_t moves = std::min(std::min(starved.size(), (size_t)max_moves), donors.size());
    const float xmax = (float)W - 1, ymax = (float)H - 1; // main.cpp:741-742
    for (size_t j = 0; j < moves; j++) {
        float* d = splats + 9 * (size_t)donors[j].i;
        float* s = splats + 9 * (size_t)starved[j].i;
        const bool along_x = !(d[2] < d[3]);
        const float sigma = glm_clamp((along_x ? d[2] : d[3]) / shrink, 1.0f, 1024.0f);
        const float co = sincos_f32(d[4], 1), si = sincos_f32(d[4], 0);
        const float ux = along_x ? co : -si, uy = along_x ? si : co;
        const float h = 0.5f * sigma;
        const float hx = h * ux, hy = h * uy;
        const float px = d[0], py = d[1];
        d[along_x ? 2 : 3] = sigma;
        for (int k = 2; k < 9; k++) s[k] = d[k];
        d[0] = glm_clamp(px - hx, 0.0f, xmax);
        d[1] = glm_clamp(py - hy, 0.0f, ymax);
        s[0] = glm_clamp(px + hx, 0.0f, xmax);
        s[1] = glm_clamp(py + hy, 0.0f, ymax);
        for (int k = 0; k < 18; k++) adams[18 * (size_t)donors[j].i + k] = adams[18 * (size_t)starved[j].i + k] = 0.0f;
        changed_ids[2 * j] = donors[j].i;
        changed_ids[2 * j + 1] = starved[j].i;
    }
    return (int)moves;
}

// Rules 1-2 alone, for s2d_reseed, which needs no donors: the starved splats -- w < min_weight --
// ordered by (w ascending, index ascending), the first max_moves of them -> ids (room for min(max_moves, n) entries).
// Returns their number.  Where donors are plentiful these are the starved rows of density_plan, in its order.
static inline int density_starved(int n, const float* stats, int passes, int max_moves, float min_weight, int32_t* ids)
{
    if (n <= 0 || passes <= 0 || max_moves <= 0) return 0;
    struct Key {
        double v;
        int i;
    };
    std::vector<Key> starved;
    for (int i = 0; i < n; i++) {
        const double w = (double)stats[3 * (size_t)i + 2] / (double)passes;
        if (w < (double)min_weight) starved.push_back(Key{w, i});
    }
    std::sort(starved.begin(), starved.end(), [](const Key& x, const Key& y) { return x.v < y.v || (x.v == y.v && x.i < y.i); });
    const size_t kept = std::min(starved.size(), (size_t)max_moves);
    for (size_t j = 0; j < kept; j++) ids[j] = starved[j].i;
    return (int)kept;
}

} // namespace s2d
