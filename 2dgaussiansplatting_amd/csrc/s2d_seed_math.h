// s2d_seed_math.h -- the per-pixel and per-row arithmetic of importance-sampled placement (include/splat2d.h, s2d_seed_*;
// DESIGN.md section 14).  Pure functions, compiled by hipcc into the kernels of s2d_seed.hip and by g++ into the tests' shim
// (tests/hostcheck/s2d_seed_check.cpp), with -ffp-contract=off in both: every float expression is a chain of single fp32
// operations in the order written, so a NumPy restatement gives the same bits.
//
//   measure s in [0, 1]  ->  q0 = (uint32)(s * 4095 + 0.5)  ->  [S2D_SEED_SQUARED: q0 = q0 * q0 >> 12]  ->  q = q0 + floor
//   draw of row i:  (a) = pcg3d(i, 2 seed, 0x5EED5EED), (b) = pcg3d(i, 2 seed + 1, 0x5EED5EED);
//                   u = ((a.x * 2^32 + a.y) * total) >> 64;  the pixel is the first whose inclusive prefix sum of q exceeds u
//   the row:        pos = pixel + (b.x, b.y) / 2^32 clamped to the image, sx = sy = scale, rot = pi * a.z / 2^32,
//                   colour = the target's at the pixel clamped to [0, 1], opacity as given.
#pragma once

#include "s2d_math.h"

namespace s2d {

constexpr uint32_t kSeedQMax = 4095u;       // the measure's resolution, and the largest uniform share (`floor`)
constexpr uint32_t kSeedStream = 0x5EED5EEDu; // third word of both draws: no draw of init_splat (0xFFFFFFFF) is repeated

S2D_HD float seed_unit(float v) { return v < 1.0f ? v : 1.0f; } // min(1, v) for v >= 0 (a NaN counts as 1: no conversion of a NaN below)

// S2D_SEED_TARGET_EDGES: central differences of the target, indices clamped to the image.  l, r, u, d: rgb of the pixels to
// the left, right, above and below.
S2D_HD float seed_measure_edges(const float* l, const float* r, const float* u, const float* d)
{
    const float er = ::fabsf(r[0] - l[0]) + ::fabsf(d[0] - u[0]);
    const float eg = ::fabsf(r[1] - l[1]) + ::fabsf(d[1] - u[1]);
    const float eb = ::fabsf(r[2] - l[2]) + ::fabsf(d[2] - u[2]);
    const float m = (er + eg) + eb;
    return seed_unit(m * 0.5f);
}

// S2D_SEED_ERROR: x = image0, y = imageRef at the pixel.
S2D_HD float seed_measure_error(const float* x, const float* y)
{
    const float m = (::fabsf(x[0] - y[0]) + ::fabsf(x[1] - y[1])) + ::fabsf(x[2] - y[2]);
    return seed_unit(m * (1.0f / 3.0f));
}

// S2D_SEED_CALLER: the caller's value clamped to [0, 1], NaN -> 0.
S2D_HD float seed_measure_caller(float v) { return v > 0.0f ? seed_unit(v) : 0.0f; }

S2D_HD uint32_t seed_quantise(float s, bool squared, uint32_t floor_q)
{
    uint32_t q0 = (uint32_t)(s * 4095.0f + 0.5f);
    if (squared) q0 = (q0 * q0) >> 12;
    return q0 + floor_q;
}

S2D_HD uint64_t seed_mul_hi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

struct SeedDraw {
    uint64_t u;          // in [0, total): where the row falls in the cumulative importance
    uint32_t bx, by, az; // sub-pixel offset and rotation words
};

S2D_HD SeedDraw seed_draw(uint32_t i, uint32_t seed, uint64_t total)
{
    uint32_t ax = i, ay = 2u * seed, az = kSeedStream;
    uint32_t bx = i, by = 2u * seed + 1u, bz = kSeedStream;
    pcg3d(ax, ay, az);
    pcg3d(bx, by, bz);
    SeedDraw d;
    d.u = seed_mul_hi(((uint64_t)ax << 32) | (uint64_t)ay, total);
    d.bx = bx, d.by = by, d.az = az;
    return d;
}

// sx = sy of every row written: the caller's scale, or (0) the side of the square a splat would own, clamped like main.cpp:744-745.
S2D_HD float seed_scale(float scale, int W, int H, int n_splats)
{
    if (scale == 0.0f) scale = ::sqrtf((float)W * (float)H / (float)n_splats);
    return glm_clamp(scale, 1.0f, 1024.0f);
}

S2D_HD float seed_opacity(float opacity) { return opacity == 0.0f ? 1.0f : opacity; }

// The nine parameters of a row drawn at pixel (x, y); rgb: the target there.  The rasteriser's pixel centre is x + 0.5.
S2D_HD void seed_row(int x, int y, const SeedDraw& d, int W, int H, float scale, float opacity, const float* rgb, float* out9)
{
    const float denom = 4294967296.0f;
    const float pi = 3.14159265358979323846264338327950288f;
    out9[0] = glm_clamp((float)x + (float)d.bx / denom, 0.0f, (float)W - 1.0f);
    out9[1] = glm_clamp((float)y + (float)d.by / denom, 0.0f, (float)H - 1.0f);
    out9[2] = scale;
    out9[3] = scale;
    out9[4] = pi * ((float)d.az / denom);
    out9[5] = glm_clamp(rgb[0], 0.0f, 1.0f);
    out9[6] = glm_clamp(rgb[1], 0.0f, 1.0f);
    out9[7] = glm_clamp(rgb[2], 0.0f, 1.0f);
    out9[8] = opacity;
}

} // namespace s2d
