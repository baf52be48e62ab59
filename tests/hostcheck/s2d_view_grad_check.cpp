// s2d_view_grad_check.cpp -- TEST SHIM.  Compiles view_row_adjoint (2dgaussiansplatting_amd/csrc/s2d_view_math.h, the very
// function view_adjoint_kernel of s2d_view_gradient.hip calls) for the host, so that tests/test_view_grad_cpu.py can hold it to
// the NumPy restatement tests/view_grad_ref.py.  Not a fallback: the product never links this.
#include "../../2dgaussiansplatting_amd/csrc/s2d_view_math.h"

extern "C" void vgc_adjoint(const float* in, const float* g_view, int n, float origin_x, float origin_y, float zoom, float filter_var,
                            int samples, float* g_out)
{
    const s2d::ViewXform x = s2d::view_xform(origin_x, origin_y, zoom, filter_var, samples);
    for (int i = 0; i < n; i++) s2d::view_row_adjoint(x, in + 9 * (size_t)i, g_view + 9 * (size_t)i, g_out + 9 * (size_t)i);
}
