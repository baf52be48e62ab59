// s2d_density_main.cpp -- TEST PROGRAM.  The relocation planner (2dgaussiansplatting_amd/csrc/s2d_density.h) behind a main()
// of its own, so that it can be built with -fsanitize=address,undefined and run as a child process
// (tests/test_density_plan_cpu.py): nothing sanitised is ever loaded into Python.
//   s2d_density_main in.bin out.bin
// in:  int32 n, passes, max_moves, W, H; float min_weight, shrink; float stats[n*3], splats[n*9], adams[n*18]
// out: int32 moves; int32 ids[2*moves]; float splats[n*9], adams[n*18]
// The arrays are exactly as large as the planner's contract says, on the heap, so that a read or write past them is seen.
#include "../../2dgaussiansplatting_amd/csrc/s2d_density.h"

#include <cstdio>
#include <cstdlib>
#include <memory>

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[5];
    float par[2];
    if (std::fread(head, sizeof(head), 1, f) != 1 || std::fread(par, sizeof(par), 1, f) != 1) return 2;
    const int n = head[0], passes = head[1], max_moves = head[2], W = head[3], H = head[4];
    if (n < 0) return 2;
    const size_t un = (size_t)n;
    const size_t room = max_moves > 0 ? 2 * std::min<size_t>((size_t)max_moves, un) : 0;
    std::unique_ptr<float[]> stats(new float[un * 3]), splats(new float[un * 9]), adams(new float[un * 18]);
    std::unique_ptr<int32_t[]> ids(new int32_t[room]);
    if (std::fread(stats.get(), sizeof(float), un * 3, f) != un * 3 || std::fread(splats.get(), sizeof(float), un * 9, f) != un * 9 ||
        std::fread(adams.get(), sizeof(float), un * 18, f) != un * 18)
        return 2;
    std::fclose(f);
    const int32_t moves = s2d::density_plan(n, stats.get(), passes, max_moves, par[0], par[1], W, H, splats.get(), adams.get(), ids.get());
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(&moves, sizeof(moves), 1, o);
    std::fwrite(ids.get(), sizeof(int32_t), 2 * (size_t)moves, o);
    std::fwrite(splats.get(), sizeof(float), un * 9, o);
    std::fwrite(adams.get(), sizeof(float), un * 18, o);
    return std::fclose(o) == 0 ? 0 : 2;
}
