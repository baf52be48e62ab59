// s2d_api_test.hip -- the test hooks of include/splat2d_test.h: device routines on their own, without a context.
#include "../../include/splat2d.h"
#include "../../include/splat2d_test.h"

#include "s2d_device.h"
#include "s2d_owned.h"

using namespace s2d;

// (no context, so no message: a failing runtime call is S2D_E_HIP; the owners free on every way out)
#define S2D_TEST_HIP(expr)                            \
    do {                                              \
        if ((expr) != hipSuccess) return S2D_E_HIP;   \
    } while (0)

namespace {

// What both sort hooks start from, on `device`: the two key and value buffers of the sort with the caller's pairs in the
// first of each, and the sort's workspace.
struct SortRig {
    DevBuf<uint32_t> k[2], v[2], temp;
    uint32_t *ko = nullptr, *vo = nullptr; // where the sort left the result

    int create(int32_t device, const uint32_t* keys, const uint32_t* values, int64_t n)
    {
        S2D_TEST_HIP(hipSetDevice(device));
        for (int i = 0; i < 2; i++) {
            S2D_TEST_HIP(k[i].alloc((size_t)n));
            S2D_TEST_HIP(v[i].alloc((size_t)n));
        }
        S2D_TEST_HIP(temp.alloc(sort_temp_words(n)));
        S2D_TEST_HIP(hipMemcpy(k[0], keys, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
        S2D_TEST_HIP(hipMemcpy(v[0], values, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
        return S2D_OK;
    }
};

} // namespace

extern "C" {

int s2d_test_sincos(int32_t device, const float* x, int32_t n, float* sin_out, float* cos_out)
{
    if (!x || !sin_out || !cos_out || n < 0) return S2D_E_INVALID;
    DevBuf<float> dx, ds, dc;
    S2D_TEST_HIP(hipSetDevice(device));
    S2D_TEST_HIP(dx.alloc((size_t)n));
    S2D_TEST_HIP(ds.alloc((size_t)n));
    S2D_TEST_HIP(dc.alloc((size_t)n));
    S2D_TEST_HIP(hipMemcpy(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    S2D_TEST_HIP(launch_test_sincos(dx, n, ds, dc, nullptr));
    S2D_TEST_HIP(hipDeviceSynchronize());
    S2D_TEST_HIP(hipMemcpy(sin_out, ds, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    S2D_TEST_HIP(hipMemcpy(cos_out, dc, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return S2D_OK;
}

int s2d_test_sort_pairs(int32_t device, uint32_t* keys, uint32_t* values, int64_t n, int32_t key_bits)
{
    if (!keys || !values || n < 0 || key_bits < 0 || key_bits > 32) return S2D_E_INVALID;
    SortRig r;
    if (int rc = r.create(device, keys, values, n)) return rc;
    S2D_TEST_HIP(sort_pairs_u32(r.k[0], r.v[0], r.k[1], r.v[1], n, key_bits, r.temp, &r.ko, &r.vo, nullptr, nullptr));
    S2D_TEST_HIP(hipDeviceSynchronize());
    S2D_TEST_HIP(hipMemcpy(keys, r.ko, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    S2D_TEST_HIP(hipMemcpy(values, r.vo, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return S2D_OK;
}

// The generic builder's last steps (TileLists::finish): the sort whose last pass records where every key's pairs begin
// instead of writing the sorted keys, then the offsets from those.  Keys must be tile ids, < num_keys: the last pass
// indexes tile_first with the whole key.
int s2d_test_sort_tile_offsets(int32_t device, const uint32_t* keys, uint32_t* values, int64_t n, int32_t num_keys,
                               uint32_t* tile_off)
{
    if (!keys || !values || !tile_off || n < 0 || n > 0xFFFFFFFFll || num_keys < 2 || num_keys > (1 << 30)) return S2D_E_INVALID;
    for (int64_t i = 0; i < n; i++)
        if (keys[i] >= (uint32_t)num_keys) return S2D_E_INVALID;
    int key_bits = 0;
    while ((1 << key_bits) < num_keys) key_bits++;
    SortRig r;
    DevBuf<uint32_t> first, off;
    if (int rc = r.create(device, keys, values, n)) return rc;
    S2D_TEST_HIP(first.alloc(((size_t)1 << key_bits) + tile_first_temp_words(num_keys)));
    S2D_TEST_HIP(off.alloc((size_t)num_keys + 1));
    S2D_TEST_HIP(hipMemsetAsync(first, 0xFF, ((size_t)1 << key_bits) * sizeof(uint32_t), nullptr));
    S2D_TEST_HIP(sort_pairs_u32(r.k[0], r.v[0], r.k[1], r.v[1], n, key_bits, r.temp, &r.ko, &r.vo, first, nullptr));
    S2D_TEST_HIP(launch_tile_offsets_from_first(first, num_keys, (uint32_t)n, first + ((size_t)1 << key_bits), off, nullptr));
    S2D_TEST_HIP(hipDeviceSynchronize());
    S2D_TEST_HIP(hipMemcpy(values, r.vo, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    S2D_TEST_HIP(hipMemcpy(tile_off, off, ((size_t)num_keys + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return S2D_OK;
}

int s2d_test_exclusive_scan(int32_t device, uint32_t* data, int64_t n, uint64_t* total)
{
    if (!data || n < 0) return S2D_E_INVALID;
    DevBuf<uint32_t> d, temp, tot;
    uint32_t htot = 0;
    S2D_TEST_HIP(hipSetDevice(device));
    S2D_TEST_HIP(d.alloc((size_t)n));
    S2D_TEST_HIP(temp.alloc(scan_temp_words(n)));
    S2D_TEST_HIP(tot.alloc(1));
    S2D_TEST_HIP(hipMemcpy(d, data, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    S2D_TEST_HIP(exclusive_scan_u32(d, d, n, temp, tot, nullptr));
    S2D_TEST_HIP(hipDeviceSynchronize());
    S2D_TEST_HIP(hipMemcpy(data, d, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    S2D_TEST_HIP(hipMemcpy(&htot, tot, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (total) *total = htot;
    return S2D_OK;
}

} // extern "C"
