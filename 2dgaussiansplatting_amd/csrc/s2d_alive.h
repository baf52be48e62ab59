// s2d_alive.h -- device side of the alive set (include/splat2d.h, s2d_set_alive / s2d_prune / s2d_grow; DESIGN.md section
// 16): launch declarations of s2d_alive.hip.  The set itself is SplatState's (s2d_state.h): the flags project_kernel reads
// as `held`, the ascending id list the Adam kernels walk.  Every kernel here is one thread per row with byte and word
// accesses, no atomics, and does not care about the wave size.
#pragma once

#include "s2d_device.h"

namespace s2d {

// flags[i] = (src[i] != 0) != invert, the input of the scan that places the rows of a compact list.  held != nullptr: the same
// as a 0 / 1 byte (src may be held itself).  grads != nullptr: the gradient record of a row whose flag is 0 becomes +0 (nine
// words), so that a row that comes alive later starts from what main.cpp:550 gives everyone.
hipError_t launch_alive_flags(const uint8_t* src, int invert, int n, uint8_t* held, uint32_t* flags, float* grads, hipStream_t stream);

// The prune criteria (s2d_prune_config), in place: held[i] = held[i] && !(starved || faint),
//   starved: min_weight > 0 && (double)stats[3 i + 2] / (double)passes < (double)min_weight   (stats: n x 3, s2d_density)
//   faint:   min_opacity > 0 && splats[9 i + 8] < min_opacity
// A NaN on the left of either comparison prunes nothing.  stats may be null when min_weight == 0.
struct AlivePruneArgs {
    uint8_t* held = nullptr;
    const float* stats = nullptr;
    const float* splats = nullptr;
    int n = 0, passes = 0;
    float min_weight = 0.0f, min_opacity = 0.0f;
};
hipError_t launch_alive_prune(const AlivePruneArgs& a, hipStream_t stream);

// The dead rows of lowest index come alive: pos = the exclusive scan of the dead flags (launch_alive_flags with invert);
// a dead row with pos[i] < limit gets held[i] = 1 and is named in ids_out[pos[i]] (ascending; min(limit, dead) entries).
hipError_t launch_alive_pick_dead(uint8_t* held, const uint32_t* pos, int n, uint32_t limit, int32_t* ids_out, hipStream_t stream);

// ids[pos[i]] = i for rows with held[i] != 0 (s2d_halo.hip's kernel, which slab ownership builds its list with).
hipError_t launch_held_ids(const uint8_t* held, const uint32_t* pos, int n, uint32_t* ids, hipStream_t stream);

} // namespace s2d
