// s2d_view_math.h -- the arithmetic of view rendering (include/splat2d.h, s2d_view_splats / s2d_render_view; DESIGN.md
// section 17): the record transform, the supersampling resolve, the 8-bit quantiser and what a configuration is refused for.
// Pure functions, compiled by hipcc into the kernels of s2d_view.hip and by g++ into the tests' shim
// (tests/hostcheck/s2d_view_check.cpp), with -ffp-contract=off in both: every float expression is a chain of single fp32
// operations in the order written, so a NumPy restatement gives the same bits.
//
//   zr = zoom * (float)s,  fr = filter_var * (float)(s * s)                       s = samples per axis
//   pos' = ((pos.x - origin_x) * zr, (pos.y - origin_y) * zr),  ax = sx * zr,  ay = sy * zr
//   fr == 0:  sx' = ax, sy' = ay, opacity' = opacity
//   else:     sx' = sqrtf(ax * ax + fr), sy' = sqrtf(ay * ay + fr), opacity' = opacity * ((ax * ay) / (sx' * sy'))
//   rot and colour unchanged; nothing is clamped.
//
// view_row_adjoint (view gradients): the gradient g' with respect to a view record, taken back to the source
// record.  With k = (ax * ay) / (sx' * sy') as above, every line one fp32 operation after the other, left to right:
//   g_pos = g'_pos * zr,  g_rot = g'_rot,  g_col = g'_col
//   fr == 0:  g_sx = g'_sx * zr,  g_sy = g'_sy * zr,  g_op = g'_op
//   else:     g_op = g'_op * k,   t = (g'_op * opacity) * k
//             g_sx = zr * (g'_sx * (ax / sx') + t * (fr / (ax * (sx' * sx'))))      (d sx'/d ax = ax / sx',
//             g_sy = zr * (g'_sy * (ay / sy') + t * (fr / (ay * (sy' * sy'))))       d opacity'/d ax = opacity * k * fr / (ax sx'^2))
#pragma once

#include "s2d_math.h"

namespace s2d {

constexpr int kViewMaxGrid = 65536; // raster grid (out * samples) per axis: what a TileRect's 16-bit tile coordinates address

struct ViewXform {
    float ox, oy; // source coordinates of the output's top-left corner
    float zr;     // raster-grid pixels per source pixel
    float fr;     // low-pass variance in raster-grid pixels^2
};

S2D_HD int view_samples(int samples) { return samples == 0 ? 1 : samples; }

S2D_HD ViewXform view_xform(float origin_x, float origin_y, float zoom, float filter_var, int samples)
{
    const int s = view_samples(samples);
    ViewXform x;
    x.ox = origin_x;
    x.oy = origin_y;
    x.zr = zoom * (float)s;
    x.fr = filter_var * (float)(s * s);
    return x;
}

// One record (pos.x, pos.y, sx, sy, rot, r, g, b, opacity) as the view rasterises it.
S2D_HD void view_row(const ViewXform& x, const float* in9, float* out9)
{
    out9[0] = (in9[0] - x.ox) * x.zr;
    out9[1] = (in9[1] - x.oy) * x.zr;
    const float ax = in9[2] * x.zr;
    const float ay = in9[3] * x.zr;
    float sx = ax, sy = ay, opacity = in9[8];
    if (!(x.fr == 0.0f)) {
        sx = sqrt_f32(ax * ax + x.fr);
        sy = sqrt_f32(ay * ay + x.fr);
        opacity = opacity * ((ax * ay) / (sx * sy));
    }
    out9[2] = sx;
    out9[3] = sy;
    out9[4] = in9[4];
    out9[5] = in9[5];
    out9[6] = in9[6];
    out9[7] = in9[7];
    out9[8] = opacity;
}

// The gradient g9_view with respect to view_row(x, in9) as the gradient with respect to in9 (the header comment has the order).
S2D_HD void view_row_adjoint(const ViewXform& x, const float* in9, const float* g9_view, float* g9_out)
{
    g9_out[0] = g9_view[0] * x.zr;
    g9_out[1] = g9_view[1] * x.zr;
    g9_out[4] = g9_view[4];
    g9_out[5] = g9_view[5];
    g9_out[6] = g9_view[6];
    g9_out[7] = g9_view[7];
    if (x.fr == 0.0f) {
        g9_out[2] = g9_view[2] * x.zr;
        g9_out[3] = g9_view[3] * x.zr;
        g9_out[8] = g9_view[8];
        return;
    }
    const float ax = in9[2] * x.zr;
    const float ay = in9[3] * x.zr;
    const float sx = sqrt_f32(ax * ax + x.fr);
    const float sy = sqrt_f32(ay * ay + x.fr);
    const float k = (ax * ay) / (sx * sy);
    const float t = (g9_view[8] * in9[8]) * k;
    g9_out[2] = x.zr * (g9_view[2] * (ax / sx) + t * (x.fr / (ax * (sx * sx))));
    g9_out[3] = x.zr * (g9_view[3] * (ay / sy) + t * (x.fr / (ay * (sy * sy))));
    g9_out[8] = g9_view[8] * k;
}

// One channel of a 2 x 2 block of samples, p_rc at row r, column c; samples = 4 applies it twice.
S2D_HD float view_resolve4(float p00, float p01, float p10, float p11) { return ((p00 + p01) + (p10 + p11)) * 0.25f; }

// (uint8)(min(max(c, 0), 1) * 255 + 0.5), NaN -> 0.
S2D_HD uint32_t view_quantise(float c)
{
    float t = c > 0.0f ? c : 0.0f; // (a NaN compares false: 0)
    t = t < 1.0f ? t : 1.0f;
    return (uint32_t)(t * 255.0f + 0.5f);
}

S2D_HD uint32_t view_pack_rgba8(float r, float g, float b)
{
    return view_quantise(r) | (view_quantise(g) << 8) | (view_quantise(b) << 16) | 0xFF000000u;
}

// With the coverage channel (S2D_CFG_COVERAGE): the alpha byte is the coverage, quantised like the colours.
S2D_HD uint32_t view_pack_rgba8(float r, float g, float b, float a)
{
    return view_quantise(r) | (view_quantise(g) << 8) | (view_quantise(b) << 16) | (view_quantise(a) << 24);
}

S2D_HD bool view_finite(float v) { return (f32_bits(v) & 0x7f800000u) != 0x7f800000u; }

// What a configuration is refused for (S2D_E_INVALID), as a message; nullptr: nothing.  format_max: the largest S2D_VIEW_*.
static inline const char* view_config_invalid(uint32_t struct_size, uint32_t expected_size, int out_width, int out_height,
                                              float origin_x, float origin_y, float zoom, float filter_var, int samples,
                                              uint32_t format, uint32_t format_max)
{
    if (struct_size != expected_size) return "wrong struct_size";
    if (samples != 0 && samples != 1 && samples != 2 && samples != 4) return "samples must be 0 (meaning 1), 1, 2 or 4";
    const int s = view_samples(samples);
    if (out_width < 1 || out_height < 1) return "out_width and out_height must be >= 1";
    if (out_width > kViewMaxGrid / s || out_height > kViewMaxGrid / s) return "out_width * samples and out_height * samples must be <= 65536";
    if (!view_finite(zoom) || !(zoom > 0.0f)) return "zoom must be finite and > 0";
    if (!view_finite(origin_x) || !view_finite(origin_y)) return "origin must be finite";
    if (!view_finite(filter_var) || !(filter_var >= 0.0f)) return "filter_var must be finite and >= 0";
    if (format > format_max) return "unknown format";
    return nullptr;
}

} // namespace s2d
