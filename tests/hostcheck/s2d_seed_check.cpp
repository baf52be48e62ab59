// s2d_seed_check.cpp -- TEST SHIM.  Compiles the shared arithmetic of importance-sampled placement
// (2dgaussiansplatting_amd/csrc/s2d_seed_math.h, the very functions the kernels of s2d_seed.hip call) and the starved-row
// selection of s2d_reseed (density_starved, csrc/s2d_density.h) for the host, so that tests/test_seed_cpu.py can hold them to
// the NumPy restatement tests/seed_ref.py.  Not a fallback: the product never links this.
#include "../../2dgaussiansplatting_amd/csrc/s2d_density.h"
#include "../../2dgaussiansplatting_amd/csrc/s2d_seed_math.h"

// q of every pixel.  ref / image0: H x W RGBA32F (image0 only for source 1); caller: H x W floats (source 2 only).
extern "C" void sc_importance(int source, const float* ref, const float* image0, const float* caller, int W, int H, int squared,
                              uint32_t floor_q, uint32_t* q)
{
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            float s;
            if (source == 0) {
                const size_t il = (size_t)y * W + (x > 0 ? x - 1 : 0), ir = (size_t)y * W + (x < W - 1 ? x + 1 : W - 1);
                const size_t iu = (size_t)(y > 0 ? y - 1 : 0) * W + x, id = (size_t)(y < H - 1 ? y + 1 : H - 1) * W + x;
                s = s2d::seed_measure_edges(ref + 4 * il, ref + 4 * ir, ref + 4 * iu, ref + 4 * id);
            } else if (source == 1) {
                s = s2d::seed_measure_error(image0 + 4 * i, ref + 4 * i);
            } else {
                s = s2d::seed_measure_caller(caller[i]);
            }
            q[i] = s2d::seed_quantise(s, squared != 0, floor_q);
        }
    }
}

// The draws of `count` rows: u[j] and (bx, by, az)[j].
extern "C" void sc_draws(const int32_t* ids, int count, uint32_t seed, uint64_t total, uint64_t* u, uint32_t* words3)
{
    for (int j = 0; j < count; j++) {
        const s2d::SeedDraw d = s2d::seed_draw((uint32_t)ids[j], seed, total);
        u[j] = d.u;
        words3[3 * j] = d.bx, words3[3 * j + 1] = d.by, words3[3 * j + 2] = d.az;
    }
}

// The rows of `count` draws that landed in the pixels px[j]; ref: H x W RGBA32F.
extern "C" void sc_rows(const int32_t* ids, const int64_t* px, int count, uint32_t seed, uint64_t total, const float* ref, int W,
                        int H, int n_splats, float scale, float opacity, float* out9)
{
    const float sc = s2d::seed_scale(scale, W, H, n_splats), op = s2d::seed_opacity(opacity);
    for (int j = 0; j < count; j++) {
        const s2d::SeedDraw d = s2d::seed_draw((uint32_t)ids[j], seed, total);
        const int y = (int)(px[j] / W), x = (int)(px[j] - (int64_t)y * W);
        s2d::seed_row(x, y, d, W, H, sc, op, ref + 4 * px[j], out9 + 9 * (size_t)j);
    }
}

extern "C" int sc_starved(int n, const float* stats, int passes, int max_moves, float min_weight, int32_t* ids)
{
    return s2d::density_starved(n, stats, passes, max_moves, min_weight, ids);
}
