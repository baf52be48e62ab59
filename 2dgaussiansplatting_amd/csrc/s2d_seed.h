// s2d_seed.h -- importance-sampled placement on the device (include/splat2d.h, s2d_importance / s2d_seed_splats /
// s2d_reseed): launch declarations of s2d_seed.hip and the owner of the map's scratch.
//
// The image is cut into SHARES of kSeedShare consecutive pixels (row-major), a share into kSeedChunks chunks of 64.  A map is
//   q[pixels]                    the importance of every pixel (s2d_seed_math.h),
//   chunk_sum[shares * 16]       the sum of each chunk (at most 64 * 8190: 32 bits),
//   share_prefix[shares]         the INCLUSIVE 64-bit prefix sums of the shares; the last one is the total.
// A draw is a binary search over share_prefix, a walk over at most 16 chunk sums and a walk over at most 64 pixels.
// No atomics: every word has one writer, and integer sums have no order.
#pragma once

#include "s2d_device.h"
#include "s2d_owned.h"

namespace s2d {

constexpr int kSeedShare = 1024;                         // pixels per workgroup of the importance kernel
constexpr int kSeedChunk = 64;                           // pixels per chunk: what one wave loads at a time
constexpr int kSeedChunks = kSeedShare / kSeedChunk;     // 16

inline size_t seed_shares(size_t pixels) { return (pixels + kSeedShare - 1) / kSeedShare; }

enum class SeedSource { TargetEdges = 0, Error = 1, Caller = 2 }; // == S2D_SEED_*

struct SeedMap {
    uint32_t* q = nullptr;
    uint32_t* chunk_sum = nullptr;
    uint64_t* share_prefix = nullptr;
    size_t pixels = 0, shares = 0;
};

struct SeedMapArgs {
    SeedSource source = SeedSource::TargetEdges;
    const void* image0 = nullptr;    // RGBA32F, or 4 x fp16 with half_images (Error only)
    const void* image_ref = nullptr; // (TargetEdges, Error)
    const float* caller = nullptr;   // H * W floats (Caller only)
    bool half_images = false;
    int W = 0, H = 0;
    bool squared = false;
    uint32_t floor_q = 0;
    SeedMap map;
};
// importance kernel + scan kernel: the whole map of the current images.
hipError_t launch_seed_map(const SeedMapArgs& a, hipStream_t stream);

struct SeedPlaceArgs {
    SeedMap map;
    uint64_t total = 0;           // > 0: share_prefix[shares - 1], as the host read it
    const int32_t* ids = nullptr; // rows to write, distinct and in range; null: rows 0 .. count - 1
    int count = 0;
    uint32_t seed = 0;
    const void* image_ref = nullptr;
    bool half_images = false;
    int W = 0, H = 0;
    float scale = 1.0f, opacity = 1.0f; // as written (seed_scale, seed_opacity)
    float* splats = nullptr;            // n x 9
    float* adams = nullptr;             // n x 18
};
hipError_t launch_seed_place(const SeedPlaceArgs& a, hipStream_t stream);

// The scratch of a map, allocated by the first call that asks for one (a context that never seeds pays nothing).
class S2D_LOCAL SeedScratch {
public:
    hipError_t ensure(size_t pixels, SeedMap* out)
    {
        const size_t shares = seed_shares(pixels);
        if (!q_) {
            S2D_TRY(q_.alloc(pixels));
            S2D_TRY(chunk_sum_.alloc(shares * kSeedChunks));
            S2D_TRY(share_prefix_.alloc(shares));
        }
        out->q = q_, out->chunk_sum = chunk_sum_, out->share_prefix = share_prefix_;
        out->pixels = pixels, out->shares = shares;
        return hipSuccess;
    }

private:
    DevBuf<uint32_t> q_, chunk_sum_;
    DevBuf<uint64_t> share_prefix_;
};

} // namespace s2d
