// s2d_multi_plan_check.cpp -- TEST SHIM.  Compiles the list arithmetic of slab ownership
// (2dgaussiansplatting_amd/csrc/s2d_multi_plan.h, the very functions the multi-device handle calls) for the host, so that
// tests/test_multi_plan_cpu.py can run them on inputs of its own.  Not a fallback: the product never links this.
// A rank's view is its n hold words (0 where it does not hold); `held` is derived from it as the handle does.
#include "../../2dgaussiansplatting_amd/csrc/s2d_multi_plan.h"

static std::vector<int32_t> held_of(const std::vector<uint32_t>& mask)
{
    std::vector<int32_t> held;
    for (size_t i = 0; i < mask.size(); i++)
        if (mask[i]) held.push_back((int32_t)i);
    return held;
}

template <typename T>
static int put(const std::vector<T>& v, T* out)
{
    std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}

extern "C" {

void mp_slab_rows(int height, int rank, int world, int32_t* out2)
{
    int r0, r1;
    s2d::slab_rows(height, rank, world, &r0, &r1);
    out2[0] = r0, out2[1] = r1;
}

// splits, offsets: world entries; send_ids: room for n * world; rows: n; src: n * world.  Returns total; *n_rows rows.
int mp_plan(const uint32_t* mask_, int n, int rank, int world, int32_t* splits_, int32_t* offsets_, int32_t* send_ids_, int32_t* rows_,
            int32_t* src_, int32_t* n_rows)
{
    const std::vector<uint32_t> mask(mask_, mask_ + n);
    std::vector<int32_t> send_ids, splits, offsets, rows, src;
    const int total = s2d::exchange_plan(mask, held_of(mask), rank, world, &send_ids, &splits, &offsets, &rows, &src);
    put(splits, splits_);
    put(offsets, offsets_);
    put(send_ids, send_ids_);
    *n_rows = put(rows, rows_);
    put(src, src_);
    return (int)send_ids.size() == total ? total : -1;
}

// mask: n words, updated in place; keep: room for n; counts: world entries; out_ids, out_mask: room for n * world, one
// segment per destination in rank order.  Returns how many ids were kept.
int mp_handover(uint32_t* mask_, const uint32_t* fresh_, int n, int rank, int world, int32_t* keep_, int32_t* counts, int32_t* out_ids_,
                uint32_t* out_mask_)
{
    std::vector<uint32_t> mask(mask_, mask_ + n);
    const std::vector<uint32_t> fresh(fresh_, fresh_ + n);
    std::vector<int32_t> keep;
    std::vector<std::vector<int32_t>> out_ids((size_t)world, std::vector<int32_t>(3, -7)); // stale contents must go
    std::vector<std::vector<uint32_t>> out_mask((size_t)world, std::vector<uint32_t>(3, 7u));
    s2d::decide_handover(&mask, fresh, held_of(mask), rank, &keep, &out_ids, &out_mask);
    put(mask, mask_);
    int at = 0;
    for (int q = 0; q < world; q++) {
        if (out_ids[(size_t)q].size() != out_mask[(size_t)q].size()) return -1;
        counts[q] = put(out_ids[(size_t)q], out_ids_ + at);
        at += put(out_mask[(size_t)q], out_mask_ + at);
    }
    return put(keep, keep_);
}

// mask: n words, updated in place; held: n_held ids and room for n_held + k.  Returns the new number of held ids.
int mp_merge(uint32_t* mask_, int n, int32_t* held_, int n_held, const int32_t* in_ids_, const uint32_t* in_mask_, int k)
{
    std::vector<uint32_t> mask(mask_, mask_ + n);
    std::vector<int32_t> held(held_, held_ + n_held);
    s2d::merge_arrivals(std::vector<int32_t>(in_ids_, in_ids_ + k), std::vector<uint32_t>(in_mask_, in_mask_ + k), &mask, &held);
    put(mask, mask_);
    return put(held, held_);
}

int mp_late(const float* sp, int k, int row_begin, int row_end) { return s2d::late_arrivals(sp, k, row_begin, row_end); }

} // extern "C"
