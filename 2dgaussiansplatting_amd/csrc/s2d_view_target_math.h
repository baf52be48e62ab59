// s2d_view_target_math.h -- the arithmetic of s2d_view_target_device (include/splat2d_coarse.h): the
// context's target seen through a view's window, as an area (box) resample.  Pure functions, compiled by hipcc into
// view_target_kernel (s2d_view_fit.hip) and by g++ into the tests' program (tests/hostcheck/s2d_view_target_main.cpp), with
// -ffp-contract=off in both: every float expression is a chain of single fp32 operations in the order written, so a NumPy
// restatement gives the same bits.
//
// Output pixel (i, j) covers the source rectangle [x0, x1) x [y0, y1), per axis
//   x0 = origin + (float)i / zoom,  x1 = origin + (float)(i + 1) / zoom
// and source pixel c the interval [c, c + 1).  The columns that can overlap are c0 = floor(x0) .. ceil(x1) - 1, cut to the image
// [0, size): a source pixel outside the image counts as 0, the black the views draw on, and is not visited.  Its weight is the
// overlap length
//   w(c) = min(x1, (float)(c + 1)) - max(x0, (float)c)
// and the pixel's value, per channel,
//   row(r) = (((0 + wx(c0) * t[r][c0]) + wx(c0 + 1) * t[r][c0 + 1]) + ...)       columns ascending
//   acc    = (((0 + wy(r0) * row(r0)) + wy(r0 + 1) * row(r0 + 1)) + ...)         rows ascending
//   out    = acc * (zoom * zoom)
// All four channels alike.  Nothing else enters: not the view's filter_var, not its samples.
#pragma once

#include "s2d_math.h"

namespace s2d {

// One thread (or one host loop) forms an output pixel, visiting 1 / zoom source pixels per axis one after the other: the entry
// points refuse a zoom below this, where a pixel would cover more than 256 x 256 of them (a whole kernel's work in a single lane).
constexpr float kViewTargetMinZoom = 1.0f / 256.0f;

struct ViewTargetSpan {
    float lo, hi;    // [x0, x1) in source coordinates
    int first, end;  // source pixels first .. end - 1 are visited (inside the image; end <= first: none)
};

// The span of output pixel i along one axis of a source of `size` pixels.
S2D_HD ViewTargetSpan view_target_span(float origin, float zoom, int i, int size)
{
    ViewTargetSpan s;
    s.lo = origin + (float)i / zoom;
    s.hi = origin + (float)(i + 1) / zoom;
    float f = floorf(s.lo), e = ceilf(s.hi);
    f = f > 0.0f ? f : 0.0f; // (a NaN cannot occur: origin and zoom are finite, zoom > 0; an infinity compares like a number)
    e = e < (float)size ? e : (float)size;
    f = f < (float)size ? f : (float)size;
    e = e > 0.0f ? e : 0.0f;
    s.first = (int)f;
    s.end = (int)e;
    return s;
}

// The overlap length of the span with source pixel c.
S2D_HD float view_target_weight(const ViewTargetSpan& s, int c)
{
    const float a = (float)c, b = (float)(c + 1);
    const float lo = s.lo > a ? s.lo : a;
    const float hi = s.hi < b ? s.hi : b;
    return hi - lo;
}

// Output pixel (i, j) of the W x H source behind `load(x, y, t)`, which writes the four channels of source pixel (x, y) to t.
template <typename Load>
S2D_HD void view_target_pixel(const Load& load, int W, int H, float origin_x, float origin_y, float zoom, int i, int j, float* out4)
{
    const ViewTargetSpan sx = view_target_span(origin_x, zoom, i, W);
    const ViewTargetSpan sy = view_target_span(origin_y, zoom, j, H);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int y = sy.first; y < sy.end; y++) {
        float row[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int x = sx.first; x < sx.end; x++) {
            const float wx = view_target_weight(sx, x);
            float t[4];
            load(x, y, t);
            for (int k = 0; k < 4; k++) row[k] = row[k] + wx * t[k];
        }
        const float wy = view_target_weight(sy, y);
        for (int k = 0; k < 4; k++) acc[k] = acc[k] + wy * row[k];
    }
    const float zz = zoom * zoom;
    for (int k = 0; k < 4; k++) out4[k] = acc[k] * zz;
}

} // namespace s2d
