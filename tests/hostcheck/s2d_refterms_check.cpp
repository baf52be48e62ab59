// s2d_refterms_check.cpp -- TEST SHIM.  Compiles the reference-order term evaluation of
// 2dgaussiansplatting_amd/csrc/s2d_math.h (reference_terms, what S2D_CFG_REFERENCE_ORDER runs per pixel) for the host, so
// that a test can compare it with the oracle bit for bit on a machine without a GPU.  Not a CPU fallback: the product
// library never links or calls this file.
#include "../../2dgaussiansplatting_amd/csrc/s2d_math.h"

#include <cstring>

using namespace s2d;

extern "C" {

// The backward chain of pixel (0, 0) of a 1 x 1 image through a stack of n splats in index order (main.cpp:552-711):
// fin3 = image0(0, 0).rgb, ref3 = imageRef(0, 0).rgb; dsplats9 (n x 9, zero on entry) receives each splat's nine terms.
// exact != 0: G = expf(-d2 / 2), the switch of main.cpp:51, through the header's expf_ref.
void rt_backward_1x1(const float* splats9, int n, const float* fin3, const float* ref3, int exact, float* dsplats9)
{
    RefPixel px = {0.0f, 0.0f, 0.0f, 1.0f};                       // main.cpp:549
    const float dL[3] = {fin3[0] - ref3[0], fin3[1] - ref3[1], fin3[2] - ref3[2]}; // main.cpp:616
    for (int i = 0; i < n; i++) {
        Splat s;
        std::memcpy(&s, splats9 + 9 * (size_t)i, sizeof(Splat));
        const Projected p = project(s);
        if (!(row_mask16(p.pos_x, p.pos_y, p.a, p.b, p.d, p.begY, p.endY, 0, 0, 1) & 1u)) continue; // main.cpp:576-598
        if (px.T < kMinThroughput) continue;                      // main.cpp:604
        const RefSplat r = {p.a, p.b, p.b, p.d, p.cosT, p.sinT, p.sx, p.sy, p.col_r, p.col_g, p.col_b, p.opacity};
        float vx, vy;
        const float d2 = quad_form_at(0.5f, 0.5f, p.pos_x, p.pos_y, r, &vx, &vy);
        const float G = exact ? expf_ref(-0.5f * d2) : gauss_from_d2(d2); // main.cpp:610 (expf_ref: the oracle's libm, bit for bit)
        float t[9];
        reference_terms(r, G, vx, vy, px, fin3[0], fin3[1], fin3[2], dL[0], dL[1], dL[2], t);
        for (int k = 0; k < 9; k++) dsplats9[9 * (size_t)i + k] += t[k]; // (a term of -0 leaves the +0 it is added to)
    }
}

// expf_ref over an array (the test compares it with the oracle's libm expf).
void rt_expf(const float* x, int n, float* out)
{
    for (int i = 0; i < n; i++) out[i] = expf_ref(x[i]);
}

} // extern "C"
