// s2d_ranges_main.cpp -- TEST PROGRAM.  The cutter of index-range rendering (2dgaussiansplatting_amd/csrc/s2d_ranges.h)
// behind a main() of its own, so that it can be built with -fsanitize=address,undefined and run as a child process
// (tests/test_index_ranges_cpu.py): nothing sanitised is ever loaded into Python.
//   s2d_ranges_main in.bin out.bin
// in:  int32 n; uint64 budget; uint32 counts[n]
// out: int32 entries; int32 cut[entries]
// counts is exactly n words on the heap, so that a read past it is seen.
#include "../../2dgaussiansplatting_amd/csrc/s2d_ranges.h"

#include <cstdio>
#include <memory>

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n;
    uint64_t budget;
    if (std::fread(&n, sizeof(n), 1, f) != 1 || std::fread(&budget, sizeof(budget), 1, f) != 1 || n < 0) return 2;
    std::unique_ptr<uint32_t[]> counts(new uint32_t[(size_t)n]);
    if (std::fread(counts.get(), sizeof(uint32_t), (size_t)n, f) != (size_t)n) return 2;
    std::fclose(f);
    const std::vector<int> r = s2d::cut_index_ranges(counts.get(), n, budget);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t entries = (int32_t)r.size();
    std::fwrite(&entries, sizeof(entries), 1, o);
    std::fwrite(r.data(), sizeof(int), r.size(), o);
    return std::fclose(o) == 0 ? 0 : 2;
}
