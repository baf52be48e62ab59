// s2d_view_target_main.cpp -- TEST PROGRAM.  Compiles view_target_pixel (2dgaussiansplatting_amd/csrc/s2d_view_target_math.h, the
// very function view_target_kernel of s2d_view_fit.hip calls) for the host behind a main() of its own, so that
// tests/test_coarse_cpu.py can hold it to the NumPy restatement (tests/coarse_ref.py) on bytes.  Built with -ffp-contract=off.
//   s2d_view_target_main <in> <out>
// in:  int32 cases, then per case int32 W, H, out_width, out_height; float origin_x, origin_y, zoom; W * H * 4 floats
// out: per case out_height * out_width * 4 floats, then out_height * out_width pairs of doubles: the sum of the x weights and of
//      the y weights of the pixel (each weight a float, added exactly enough in double)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../2dgaussiansplatting_amd/csrc/s2d_view_target_math.h"

struct HostLoad {
    const float* image;
    int W;
    void operator()(int x, int y, float* t) const
    {
        const float* p = image + ((size_t)y * (size_t)W + (size_t)x) * 4;
        for (int k = 0; k < 4; k++) t[k] = p[k];
    }
};

static double weight_sum(float origin, float zoom, int i, int size)
{
    const s2d::ViewTargetSpan s = s2d::view_target_span(origin, zoom, i, size);
    double sum = 0.0;
    for (int c = s.first; c < s.end; c++) sum += (double)s2d::view_target_weight(s, c);
    return sum;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t cases = 0;
    if (fread(&cases, sizeof cases, 1, in) != 1) return 3;
    for (int32_t k = 0; k < cases; k++) {
        int32_t dims[4];
        float win[3];
        if (fread(dims, sizeof dims, 1, in) != 1 || fread(win, sizeof win, 1, in) != 1) return 3;
        const int W = dims[0], H = dims[1], ow = dims[2], oh = dims[3];
        if (W < 1 || H < 1 || ow < 1 || oh < 1) return 3;
        std::vector<float> image((size_t)W * H * 4), view((size_t)ow * oh * 4);
        std::vector<double> sums((size_t)ow * oh * 2);
        if (fread(image.data(), sizeof(float), image.size(), in) != image.size()) return 3;
        for (int j = 0; j < oh; j++)
            for (int i = 0; i < ow; i++) {
                s2d::view_target_pixel(HostLoad{image.data(), W}, W, H, win[0], win[1], win[2], i, j, &view[((size_t)j * ow + i) * 4]);
                sums[((size_t)j * ow + i) * 2 + 0] = weight_sum(win[0], win[2], i, W);
                sums[((size_t)j * ow + i) * 2 + 1] = weight_sum(win[1], win[2], j, H);
            }
        if (fwrite(view.data(), sizeof(float), view.size(), out) != view.size()) return 4;
        if (fwrite(sums.data(), sizeof(double), sums.size(), out) != sums.size()) return 4;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
