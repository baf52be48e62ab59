// s2d_density_check.cpp -- TEST SHIM.  Compiles the relocation planner of s2d_relocate
// (2dgaussiansplatting_amd/csrc/s2d_density.h, the very function the library calls) for the host, so that tests can run it
// on inputs of their own: tests/test_density_plan_cpu.py against a NumPy restatement of its rules, and
// tests/test_gpu_density.py against what s2d_relocate did on the device.  Not a fallback: the product never links this.
#include "../../2dgaussiansplatting_amd/csrc/s2d_density.h"

extern "C" int dp_plan(int n, const float* stats, int passes, int max_moves, float min_weight, float shrink, int W, int H,
                       float* splats, float* adams, int32_t* changed_ids)
{
    return s2d::density_plan(n, stats, passes, max_moves, min_weight, shrink, W, H, splats, adams, changed_ids);
}
