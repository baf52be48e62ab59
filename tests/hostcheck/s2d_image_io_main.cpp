// s2d_image_io_main.cpp -- TEST PROGRAM.  The RGBA side of the host program's image files (2dgaussiansplatting_amd/host/image_io.h:
// load_image_rgba, save_png_rgba, premultiplied_target, quantise_straight) behind a main() of its own, built with
// -fsanitize=address,undefined and run as a child process (tests/test_coverage_cpu.py).
//   s2d_image_io_main write  w h in.rgba out.png     raw RGBA8 bytes -> an RGBA PNG
//   s2d_image_io_main read   in.(png|ppm|s2di|jpg) out.bin    -> int32 w, int32 h, then w*h*4 bytes (alpha kept, or 255)
//   s2d_image_io_main target in.png out.bin          -> int32 w, int32 h, then w*h*4 floats: the coverage target of the file
//   s2d_image_io_main straight w h in.f32 out.bin    w*h*4 floats (premultiplied colour, coverage) -> w*h*4 bytes, straight alpha
#include "../../2dgaussiansplatting_amd/host/image_io.h"

#include <memory>

static bool write_all(const char* path, const int32_t* wh, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    bool ok = !wh || std::fwrite(wh, sizeof(int32_t), 2, f) == 2;
    ok = ok && std::fwrite(data, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const std::string cmd = argv[1];
    if (cmd == "write" && argc == 6) {
        s2dio::ImageRGBA8 im;
        im.w = std::atoi(argv[2]);
        im.h = std::atoi(argv[3]);
        std::vector<uint8_t> d;
        if (im.w <= 0 || im.h <= 0 || !s2dio::read_file(argv[4], &d) || d.size() != (size_t)im.w * im.h * 4) return 2;
        im.rgba = d;
        return s2dio::save_png_rgba(argv[5], im) ? 0 : 1;
    }
    if (cmd == "read" && argc == 4) {
        s2dio::ImageRGBA8 im;
        if (!s2dio::load_image_rgba(argv[2], &im)) return 1;
        const int32_t wh[2] = {im.w, im.h};
        return write_all(argv[3], wh, im.rgba.data(), im.rgba.size()) ? 0 : 2;
    }
    if (cmd == "target" && argc == 4) {
        s2dio::ImageRGBA8 im;
        if (!s2dio::load_image_rgba(argv[2], &im)) return 1;
        const std::vector<float> t = s2dio::premultiplied_target(im);
        const int32_t wh[2] = {im.w, im.h};
        return write_all(argv[3], wh, t.data(), t.size() * sizeof(float)) ? 0 : 2;
    }
    if (cmd == "straight" && argc == 6) {
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
        std::vector<uint8_t> d;
        if (w <= 0 || h <= 0 || !s2dio::read_file(argv[4], &d) || d.size() != (size_t)w * h * 4 * sizeof(float)) return 2;
        std::vector<float> f((size_t)w * h * 4);
        std::memcpy(f.data(), d.data(), d.size());
        const s2dio::ImageRGBA8 im = s2dio::quantise_straight(f, w, h);
        return write_all(argv[5], nullptr, im.rgba.data(), im.rgba.size()) ? 0 : 2;
    }
    return 2;
}
