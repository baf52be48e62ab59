// s2d_api_placement.hip -- where splats are put from outside the optimiser, through the C ABI: the density statistics
// and s2d_relocate (s2d_density.h), importance-sampled placement (s2d_importance, s2d_seed_splats, s2d_reseed; s2d_seed.h).
#include "s2d_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "s2d_density.h" // (behind s2d_device.h: s2d_math.h's qualifiers need the HIP runtime header under hipcc)
#include "s2d_seed_math.h"

namespace {

// Host arrays handed to the context's stream as temporary device buffers: allocated, the upload queued.  The stream is
// idle before the buffers are freed and while the host arrays are read, on whichever way the function is left.
class StreamTemps {
public:
    explicit StreamTemps(hipStream_t stream) : idle_{stream} {}
    template <typename T>
    hipError_t upload(const T* host, size_t count, const T** device)
    {
        bufs_.emplace_back();
        S2D_TRY(bufs_.back().alloc(count * sizeof(T)));
        *device = reinterpret_cast<const T*>((const uint8_t*)bufs_.back());
        return hipMemcpyAsync(bufs_.back(), host, count * sizeof(T), hipMemcpyHostToDevice, idle_.stream);
    }

private:
    std::vector<DevBuf<uint8_t>> bufs_;
    IdleAtExit idle_; // (the last member: the first to go)
};

// The density statistics on their way to the host (stats: n x 3 floats; queued -- the caller waits, with whatever else it
// reads), and the number of passes they hold: S2D_E_STATE when none since the last reset.  Selects the context's device.
int density_to_host(s2d_ctx* c, const char* who, float* stats, int* passes)
{
    *passes = c->density.passes();
    if (*passes == 0) return fail(c, S2D_E_STATE, "%s needs a pass with S2D_BWD_DENSITY_STATS since the last reset", who);
    if (int rc = use_device(c)) return rc;
    if (c->n > 0) S2D_HIP(c, hipMemcpyAsync(stats, c->density.data(), (size_t)c->n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return S2D_OK;
}

// s2d_density_get (to_host: waits) and _device (queued).
int density_get(s2d_ctx* c, void* out, bool to_host, int32_t* passes)
{
    if (int rc = use_device(c)) return rc;
    const size_t bytes = (size_t)c->n * sizeof(s2d_density);
    if (out && bytes && c->density.data()) {
        if (to_host) {
            if (int rc = read_back(c, out, c->density.data(), bytes)) return rc;
        } else {
            S2D_HIP(c, hipMemcpyAsync(out, c->density.data(), bytes, hipMemcpyDeviceToDevice, c->stream));
        }
    } else if (out && bytes) { // no pass has asked yet: all zeros
        if (to_host) std::memset(out, 0, bytes);
        else S2D_HIP(c, hipMemsetAsync(out, 0, bytes, c->stream));
    }
    if (passes) *passes = c->density.passes();
    return S2D_OK;
}

} // namespace

// ---- importance-sampled placement (s2d_seed.h; declared in s2d_ctx.h) --------------------------------------------------
int seed_refused(s2d_ctx* c, const s2d_seed_config* cfg, const char* who, bool has_reference_order)
{
    if (!cfg || cfg->struct_size != sizeof(s2d_seed_config)) return fail(c, S2D_E_INVALID, "s2d_seed_config: NULL or wrong struct_size");
    if (cfg->source > S2D_SEED_CALLER) return fail(c, S2D_E_INVALID, "s2d_seed_config: unknown source %u", cfg->source);
    if (cfg->flags & ~S2D_SEED_SQUARED) return fail(c, S2D_E_INVALID, "s2d_seed_config: unknown flags 0x%x", cfg->flags);
    if (cfg->floor > kSeedQMax) return fail(c, S2D_E_INVALID, "s2d_seed_config: floor %u > 4095", cfg->floor);
    if (!(cfg->scale >= 0.0f) || std::isinf(cfg->scale)) return fail(c, S2D_E_INVALID, "s2d_seed_config: scale must be finite and >= 0 (0: sqrt(W H / n))");
    if (!(cfg->opacity >= 0.0f && cfg->opacity <= 1.0f)) return fail(c, S2D_E_INVALID, "s2d_seed_config: opacity must be 0 (meaning 1) or in (0, 1]");
    if ((cfg->source == S2D_SEED_CALLER) != (cfg->importance_device != nullptr))
        return fail(c, S2D_E_INVALID, "s2d_seed_config: importance_device goes with S2D_SEED_CALLER, and only with it");
    return whole_scene_refused(c, who, has_reference_order); // (the importance map covers the whole image)
}

int seed_state_refused(s2d_ctx* c, const s2d_seed_config* cfg)
{
    if (!c->fresh.target()) return fail(c, S2D_E_STATE, "no target image set (s2d_set_target)");
    if (cfg->source == S2D_SEED_ERROR && !c->fresh.forward())
        return fail(c, S2D_E_STATE, "S2D_SEED_ERROR needs s2d_forward on the current parameters");
    return S2D_OK;
}

int seed_map(s2d_ctx* c, const s2d_seed_config* cfg, SeedMap* map, uint64_t* total)
{
    S2D_HIP(c, c->seed.ensure(slab_pixels(c), map));
    SeedMapArgs a;
    a.source = (SeedSource)cfg->source; a.image0 = c->d_image0; a.image_ref = c->d_ref; a.caller = cfg->importance_device;
    a.half_images = c->half_images; a.W = c->g.W; a.H = c->g.H; a.squared = (cfg->flags & S2D_SEED_SQUARED) != 0; a.floor_q = cfg->floor;
    a.map = *map;
    S2D_HIP(c, launch_seed_map(a, c->stream));
    return read_back(c, total, map->share_prefix + (map->shares - 1), sizeof(uint64_t));
}

int seed_place(s2d_ctx* c, const s2d_seed_config* cfg, const SeedMap& map, uint64_t total, const int32_t* ids_device, int count)
{
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    SeedPlaceArgs p;
    p.map = map; p.total = total; p.ids = ids_device; p.count = count; p.seed = cfg->seed;
    p.image_ref = c->d_ref; p.half_images = c->half_images; p.W = c->g.W; p.H = c->g.H;
    p.scale = seed_scale(cfg->scale, c->g.W, c->g.H, c->n); p.opacity = seed_opacity(cfg->opacity);
    p.splats = now.splats; p.adams = now.adams;
    S2D_HIP(c, launch_seed_place(p, c->stream));
    return rows_replaced(c, S2D_ROWS_SPLATS);
}

int mask_dead_stats(s2d_ctx* c, float* stats)
{
    if (c->state.kind() != SplatState::Subset::Alive || c->n == 0) return S2D_OK;
    std::vector<uint8_t> alive((size_t)c->n);
    if (int rc = read_back(c, alive.data(), c->state.held(), alive.size())) return rc;
    for (size_t i = 0; i < alive.size(); i++)
        if (!alive[i]) stats[3 * i] = stats[3 * i + 1] = stats[3 * i + 2] = std::nanf("");
    return S2D_OK;
}

namespace {

// The rows `ids` (distinct, in range; null: 0 .. count - 1) drawn from the map of the current images and written
// (rows_replaced).  *placed: count, or 0 for a map whose total is 0.
int seed_rows(s2d_ctx* c, const s2d_seed_config* cfg, const int32_t* ids, int count, int32_t* placed)
{
    *placed = 0;
    SeedMap map;
    uint64_t total = 0;
    if (int rc = seed_map(c, cfg, &map, &total)) return rc;
    if (total == 0 || count == 0) return S2D_OK;
    StreamTemps tmp(c->stream);
    const int32_t* d_ids = nullptr;
    if (ids) S2D_HIP(c, tmp.upload(ids, (size_t)count, &d_ids));
    if (int rc = seed_place(c, cfg, map, total, d_ids, count)) return rc;
    *placed = count;
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_density_get_device(s2d_ctx* c, float* out_device, int32_t* passes)
{
    if (!c || (!out_device && c->n)) return S2D_E_INVALID;
    return density_get(c, out_device, false, passes);
}

int s2d_density_get(s2d_ctx* c, s2d_density* host, int32_t* passes)
{
    if (!c) return S2D_E_INVALID;
    return density_get(c, host, true, passes);
}

int s2d_density_reset(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, c->density.reset());
    return S2D_OK;
}

int s2d_relocate(s2d_ctx* c, const s2d_relocate_config* cfg, int32_t* moved)
{
    if (!c || !cfg || cfg->struct_size != sizeof(s2d_relocate_config)) return S2D_E_INVALID;
    if (moved) *moved = 0;
    const float shrink = cfg->shrink == 0.0f ? 1.6f : cfg->shrink;
    if (cfg->max_moves < 0 || !(shrink > 0.0f) || std::isinf(shrink) || std::isnan(cfg->min_weight))
        return fail(c, S2D_E_INVALID, "s2d_relocate: max_moves >= 0, a finite shrink > 0 (0: 1.6) and a min_weight that is a number");
    if (int rc = whole_scene_refused(c, "s2d_relocate", false)) return rc; // (the statistics of the whole image)
    const size_t n = (size_t)c->n;
    int passes = 0;
    std::vector<float> stats(n * 3), splats(n * 9), adams(n * 18);
    if (int rc = density_to_host(c, "s2d_relocate", stats.data(), &passes)) return rc;
    std::vector<int32_t> ids(2 * std::min<size_t>((size_t)cfg->max_moves, n));
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    if (n > 0) {
        S2D_HIP(c, hipMemcpyAsync(splats.data(), now.splats, n * 9 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        S2D_HIP(c, hipMemcpyAsync(adams.data(), now.adams, n * 18 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    S2D_HIP(c, hipStreamSynchronize(c->stream)); // (one wait for the three arrays)
    if (int rc = mask_dead_stats(c, stats.data())) return rc; // (dead rows: neither starved nor donors)
    const int moves = density_plan(c->n, stats.data(), passes, cfg->max_moves, cfg->min_weight, shrink, c->g.W, c->g.H, splats.data(),
                                   adams.data(), ids.data());
    if (moves > 0) { // the changed rows, through the row calls' scatter
        const size_t rows = 2 * (size_t)moves;
        std::vector<float> srows(rows * 9), arows(rows * 18);
        for (size_t r = 0; r < rows; r++) {
            std::memcpy(&srows[r * 9], &splats[(size_t)ids[r] * 9], 9 * sizeof(float));
            std::memcpy(&arows[r * 18], &adams[(size_t)ids[r] * 18], 18 * sizeof(float));
        }
        StreamTemps tmp(c->stream);
        const int32_t* d_ids = nullptr;
        const float *d_srows = nullptr, *d_arows = nullptr;
        S2D_HIP(c, tmp.upload(ids.data(), rows, &d_ids));
        S2D_HIP(c, tmp.upload(srows.data(), rows * 9, &d_srows));
        S2D_HIP(c, tmp.upload(arows.data(), rows * 18, &d_arows));
        S2D_HIP(c, launch_rows_scatter(now.splats, 9, d_ids, (int)rows, c->n, d_srows, c->stream));
        S2D_HIP(c, launch_rows_scatter(now.adams, 18, d_ids, (int)rows, c->n, d_arows, c->stream));
        if (int rc = rows_replaced(c, S2D_ROWS_SPLATS)) return rc;
        S2D_HIP(c, hipStreamSynchronize(c->stream)); // (the host copies are read by the stream until here)
    }
    S2D_HIP(c, c->density.reset());
    if (moved) *moved = moves;
    return S2D_OK;
}

int s2d_importance(s2d_ctx* c, const s2d_seed_config* cfg, uint32_t* q_host, uint64_t* total)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = seed_refused(c, cfg, "s2d_importance")) return rc;
    if (int rc = seed_state_refused(c, cfg)) return rc;
    if (int rc = use_device(c)) return rc;
    SeedMap map;
    uint64_t sum = 0;
    if (int rc = seed_map(c, cfg, &map, &sum)) return rc;
    if (q_host)
        if (int rc = read_back(c, q_host, map.q, map.pixels * sizeof(uint32_t))) return rc;
    if (total) *total = sum;
    return S2D_OK;
}

int s2d_seed_splats(s2d_ctx* c, const s2d_seed_config* cfg, const int32_t* ids_host, int32_t count, int32_t* placed)
{
    if (!c) return S2D_E_INVALID;
    if (placed) *placed = 0;
    if (int rc = seed_refused(c, cfg, "s2d_seed_splats")) return rc;
    if (count < 0 || count > c->n) return fail(c, S2D_E_INVALID, "s2d_seed_splats: count %d outside 0 .. n_splats", count);
    if (ids_host) {
        std::vector<bool> seen((size_t)c->n, false);
        for (int j = 0; j < count; j++) {
            const int32_t i = ids_host[j];
            if (i < 0 || i >= c->n || seen[(size_t)i]) return fail(c, S2D_E_INVALID, "s2d_seed_splats: ids[%d] = %d is out of range or repeated", j, i);
            seen[(size_t)i] = true;
        }
    }
    if (int rc = seed_state_refused(c, cfg)) return rc;
    if (int rc = use_device(c)) return rc;
    int32_t done = 0;
    if (int rc = seed_rows(c, cfg, ids_host, count, &done)) return rc;
    if (placed) *placed = done;
    return S2D_OK;
}

int s2d_reseed(s2d_ctx* c, const s2d_seed_config* cfg, int32_t max_moves, float min_weight, int32_t* moved)
{
    if (!c) return S2D_E_INVALID;
    if (moved) *moved = 0;
    if (int rc = seed_refused(c, cfg, "s2d_reseed", false)) return rc;
    if (max_moves < 0 || std::isnan(min_weight)) return fail(c, S2D_E_INVALID, "s2d_reseed: max_moves >= 0 and a min_weight that is a number");
    if (int rc = seed_state_refused(c, cfg)) return rc;
    int passes = 0;
    std::vector<float> stats((size_t)c->n * 3);
    if (int rc = density_to_host(c, "s2d_reseed", stats.data(), &passes)) return rc;
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = mask_dead_stats(c, stats.data())) return rc; // (dead rows are not starved)
    std::vector<int32_t> ids(std::min<size_t>((size_t)max_moves, (size_t)c->n));
    const int starved = density_starved(c->n, stats.data(), passes, max_moves, min_weight, ids.data());
    int32_t done = 0;
    if (starved > 0)
        if (int rc = seed_rows(c, cfg, ids.data(), starved, &done)) return rc;
    S2D_HIP(c, c->density.reset());
    if (moved) *moved = done;
    return S2D_OK;
}

} // extern "C"
