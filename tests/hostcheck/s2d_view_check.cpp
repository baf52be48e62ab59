// s2d_view_check.cpp -- TEST SHIM.  Compiles the shared arithmetic of view rendering
// (2dgaussiansplatting_amd/csrc/s2d_view_math.h, the very functions the kernels of s2d_view.hip and the entry points of
// s2d_api_view.hip call) for the host, so that tests/test_view_cpu.py can hold them to the NumPy restatement
// tests/view_ref.py.  Not a fallback: the product never links this.
#include "../../include/splat2d.h"
#include "../../2dgaussiansplatting_amd/csrc/s2d_view_math.h"

extern "C" unsigned vc_config_size(void) { return (unsigned)sizeof(s2d_view_config); }

// 1: the configuration is refused (S2D_E_INVALID), 0: not.
extern "C" int vc_refused(const s2d_view_config* c)
{
    return s2d::view_config_invalid(c->struct_size, (uint32_t)sizeof(s2d_view_config), c->out_width, c->out_height, c->origin_x,
                                    c->origin_y, c->zoom, c->filter_var, c->samples, c->format, S2D_VIEW_RGBA8) != nullptr;
}

extern "C" void vc_rows(const float* in, int n, float origin_x, float origin_y, float zoom, float filter_var, int samples, float* out)
{
    const s2d::ViewXform x = s2d::view_xform(origin_x, origin_y, zoom, filter_var, samples);
    for (int i = 0; i < n; i++) s2d::view_row(x, in + 9 * (size_t)i, out + 9 * (size_t)i);
}

// One level of the resolve: in (2h) x (2w) RGBA32F -> out h x w RGBA32F, .w = 1.
extern "C" void vc_resolve2(const float* in, int w, int h, float* out)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const float* p00 = in + 4 * ((size_t)(2 * y) * (2 * w) + 2 * x);
            const float* p10 = p00 + 4 * (size_t)(2 * w);
            float* o = out + 4 * ((size_t)y * w + x);
            for (int k = 0; k < 3; k++) o[k] = s2d::view_resolve4(p00[k], p00[4 + k], p10[k], p10[4 + k]);
            o[3] = 1.0f;
        }
}

// pixels RGBA32F -> RGBA8 words
extern "C" void vc_quantise(const float* in, size_t pixels, uint32_t* out)
{
    for (size_t i = 0; i < pixels; i++) out[i] = s2d::view_pack_rgba8(in[4 * i], in[4 * i + 1], in[4 * i + 2]);
}
