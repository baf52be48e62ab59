// s2d_multi_plan_main.cpp -- TEST PROGRAM.  The list arithmetic of slab ownership (2dgaussiansplatting_amd/csrc/s2d_multi_plan.h)
// behind a main() of its own, so that it can be built with -fsanitize=address,undefined and run as a child process
// (tests/test_multi_plan_cpu.py): nothing sanitised is ever loaded into Python.
//   s2d_multi_plan_main in.bin out.bin
// in: records until the end of the file, each int32 op, int32 a, b, c and then the arrays of the op (32-bit words):
//   1 slab rows   a = height, b = rank, c = world                                  -> r0, r1
//   2 plan        a = n, b = rank, c = world; mask[n]                              -> total, n_rows, splits[world], offsets[world],
//                                                                                     send_ids[total], rows[n_rows], src[n_rows * world]
//   3 hand-over   a = n, b = rank, c = world; mask[n], fresh[n]                    -> mask[n], n_keep, keep[n_keep], counts[world],
//                                                                                     out_ids[sum], out_mask[sum]
//   4 merge       a = n, b = n_held, c = k; mask[n], held[n_held], in_ids[k], in_mask[k] -> mask[n], n_held, held[n_held]
//   5 late count  a = k, b = row_begin, c = row_end; sp[9 k] (float)               -> count
// Every input array is exactly its size on the heap, every output array exactly the room the shim's comment asks for,
// so that a read or write past either is seen.
#include "s2d_multi_plan_check.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

typedef std::unique_ptr<int32_t[]> Words;

static Words read_words(FILE* f, size_t count)
{
    Words w(new int32_t[count]);
    if (std::fread(w.get(), 4, count, f) != count) std::exit(2);
    return w;
}

static void write_words(FILE* o, const void* p, size_t count)
{
    if (std::fwrite(p, 4, count, o) != count) std::exit(2);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    FILE* o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int32_t head[4];
    while (std::fread(head, 4, 4, f) == 4) {
        const int32_t op = head[0], a = head[1], b = head[2], c = head[3];
        if (a < 0 || b < 0 || c < 0) return 2;
        if (op == 1) {
            int32_t r[2];
            mp_slab_rows(a, b, c, r);
            write_words(o, r, 2);
        } else if (op == 2) {
            const size_t n = (size_t)a, world = (size_t)c;
            Words mask = read_words(f, n), splits(new int32_t[world]), offsets(new int32_t[world]), send_ids(new int32_t[n * world]),
                  rows(new int32_t[n]), src(new int32_t[n * world]);
            int32_t n_rows = 0;
            const int32_t total = mp_plan((const uint32_t*)mask.get(), a, b, c, splits.get(), offsets.get(), send_ids.get(), rows.get(), src.get(), &n_rows);
            if (total < 0) return 3;
            write_words(o, &total, 1);
            write_words(o, &n_rows, 1);
            write_words(o, splits.get(), world);
            write_words(o, offsets.get(), world);
            write_words(o, send_ids.get(), (size_t)total);
            write_words(o, rows.get(), (size_t)n_rows);
            write_words(o, src.get(), (size_t)n_rows * world);
        } else if (op == 3) {
            const size_t n = (size_t)a, world = (size_t)c;
            Words mask = read_words(f, n), fresh = read_words(f, n), keep(new int32_t[n]), counts(new int32_t[world]), ids(new int32_t[n * world]),
                  words(new int32_t[n * world]);
            const int32_t n_keep = mp_handover((uint32_t*)mask.get(), (const uint32_t*)fresh.get(), a, b, c, keep.get(), counts.get(), ids.get(),
                                               (uint32_t*)words.get());
            if (n_keep < 0) return 3;
            size_t sum = 0;
            for (size_t q = 0; q < world; q++) sum += (size_t)counts[q];
            write_words(o, mask.get(), n);
            write_words(o, &n_keep, 1);
            write_words(o, keep.get(), (size_t)n_keep);
            write_words(o, counts.get(), world);
            write_words(o, ids.get(), sum);
            write_words(o, words.get(), sum);
        } else if (op == 4) {
            const size_t n = (size_t)a, n_held = (size_t)b, k = (size_t)c;
            Words mask = read_words(f, n), held(new int32_t[n_held + k]);
            if (std::fread(held.get(), 4, n_held, f) != n_held) return 2;
            Words in_ids = read_words(f, k), in_mask = read_words(f, k);
            const int32_t now = mp_merge((uint32_t*)mask.get(), a, held.get(), b, in_ids.get(), (const uint32_t*)in_mask.get(), c);
            write_words(o, mask.get(), n);
            write_words(o, &now, 1);
            write_words(o, held.get(), (size_t)now);
        } else if (op == 5) {
            std::unique_ptr<float[]> sp(new float[(size_t)a * 9]);
            if (std::fread(sp.get(), 4, (size_t)a * 9, f) != (size_t)a * 9) return 2;
            const int32_t late = mp_late(sp.get(), a, b, c);
            write_words(o, &late, 1);
        } else {
            return 2;
        }
    }
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
