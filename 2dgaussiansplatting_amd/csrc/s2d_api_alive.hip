// s2d_api_alive.hip -- the alive set through the C ABI (include/splat2d.h): s2d_set_alive,
// s2d_set_alive_device, s2d_get_alive, s2d_prune, s2d_grow.  The set is SplatState's (s2d_state.h), the kernels are
// s2d_alive.hip's; every change ends in the event alive_set_changed (s2d_sequence.h).
#include "s2d_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "s2d_alive.h"

namespace {

// What all five calls refuse, before any device work: a dead row is a notion of one context that draws the whole image.
int alive_refused(s2d_ctx* c, const char* who)
{
    if (c->g.row_begin != 0 || c->g.row_end != c->g.H) return fail(c, S2D_E_INVALID, "%s: not available for a row slab context", who);
    if (c->state.kind() == SplatState::Subset::Slab)
        return fail(c, S2D_E_INVALID, "%s: this context holds a subset by slab ownership (s2d_halo_commit)", who);
    if (c->cfg.flags & S2D_CFG_REFERENCE_ORDER) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_REFERENCE_ORDER", who);
    return S2D_OK;
}

bool has_set(const s2d_ctx* c) { return c->state.kind() == SplatState::Subset::Alive; }

// The mask from host (waits: the caller's array is read by the stream until then) or device memory (queued); null: none.
int set_alive(s2d_ctx* c, const char* who, const uint8_t* mask, bool from_host)
{
    if (int rc = alive_refused(c, who)) return rc;
    if (int rc = use_device(c)) return rc;
    if (!mask) {
        if (!has_set(c)) return S2D_OK;
        S2D_HIP(c, c->state.clear_alive());
        alive_set_changed(c);
        return S2D_OK;
    }
    uint8_t* flags = nullptr;
    S2D_HIP(c, c->state.begin_alive(&flags, c->d_scan_temp));
    if (c->n > 0) S2D_HIP(c, hipMemcpyAsync(flags, mask, (size_t)c->n, from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    S2D_HIP(c, c->state.finish_alive(c->d_grads, c->d_scan_temp));
    alive_set_changed(c);
    if (from_host) {
        S2D_HIP(c, hipStreamSynchronize(c->stream));
        int count = 0;
        for (int i = 0; i < c->n; i++) count += mask[i] != 0;
        c->state.alive_count_is(count);
    }
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_set_alive(s2d_ctx* c, const uint8_t* alive_host)
{
    if (!c) return S2D_E_INVALID;
    return set_alive(c, "s2d_set_alive", alive_host, true);
}

int s2d_set_alive_device(s2d_ctx* c, const uint8_t* alive_device)
{
    if (!c) return S2D_E_INVALID;
    return set_alive(c, "s2d_set_alive_device", alive_device, false);
}

int s2d_get_alive(s2d_ctx* c, uint8_t* alive_host, int32_t* count)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = alive_refused(c, "s2d_get_alive")) return rc;
    if (!has_set(c)) {
        if (alive_host) std::memset(alive_host, 1, (size_t)c->n);
        if (count) *count = c->n;
        return S2D_OK;
    }
    if (int rc = use_device(c)) return rc;
    if (alive_host && c->n > 0)
        if (int rc = read_back(c, alive_host, c->state.held(), (size_t)c->n)) return rc;
    if (count) {
        int k = 0;
        S2D_HIP(c, c->state.alive_count(&k));
        *count = k;
    }
    return S2D_OK;
}

int s2d_prune(s2d_ctx* c, const s2d_prune_config* cfg, int32_t* pruned)
{
    if (!c) return S2D_E_INVALID;
    if (pruned) *pruned = 0;
    if (!cfg || cfg->struct_size != sizeof(s2d_prune_config)) return fail(c, S2D_E_INVALID, "s2d_prune_config: NULL or wrong struct_size");
    if (!(cfg->min_weight >= 0.0f) || !(cfg->min_opacity >= 0.0f) || (cfg->min_weight == 0.0f && cfg->min_opacity == 0.0f))
        return fail(c, S2D_E_INVALID, "s2d_prune_config: thresholds are numbers >= 0, and not both 0");
    if (int rc = alive_refused(c, "s2d_prune")) return rc;
    const bool by_weight = cfg->min_weight > 0.0f;
    if (by_weight && c->density.passes() == 0)
        return fail(c, S2D_E_STATE, "s2d_prune with min_weight needs a pass with S2D_BWD_DENSITY_STATS since the last reset");
    if (int rc = use_device(c)) return rc;
    int before = 0, after = 0;
    S2D_HIP(c, c->state.alive_count(&before));
    AlivePruneArgs a;
    S2D_HIP(c, c->state.begin_alive(&a.held, c->d_scan_temp));
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    a.stats = by_weight ? c->density.data() : nullptr; a.splats = now.splats; a.n = c->n; a.passes = c->density.passes();
    a.min_weight = cfg->min_weight; a.min_opacity = cfg->min_opacity;
    S2D_HIP(c, launch_alive_prune(a, c->stream));
    S2D_HIP(c, c->state.finish_alive(c->d_grads, c->d_scan_temp));
    S2D_HIP(c, c->state.alive_count(&after)); // (the one read-back, where the host knew the count before)
    if (after != before) alive_set_changed(c); // (the same rows alive: lists and projection stand)
    if (by_weight) S2D_HIP(c, c->density.reset());
    if (pruned) *pruned = before - after;
    return S2D_OK;
}

int s2d_grow(s2d_ctx* c, const s2d_seed_config* cfg, const int32_t* ids_host, int32_t count, int32_t* grown)
{
    if (!c) return S2D_E_INVALID;
    if (grown) *grown = 0;
    if (int rc = alive_refused(c, "s2d_grow")) return rc;
    if (int rc = seed_refused(c, cfg, "s2d_grow")) return rc;
    if (count < 0) return fail(c, S2D_E_INVALID, "s2d_grow: count %d < 0", count);
    const int n = c->n;
    std::vector<uint8_t> mask; // explicit ids: the set as it will be
    if (ids_host && count > 0) {
        if (count > n) return fail(c, S2D_E_INVALID, "s2d_grow: count %d > n_splats", count);
        mask.assign((size_t)n, 1);
        if (has_set(c)) {
            if (int rc = use_device(c)) return rc;
            if (int rc = read_back(c, mask.data(), c->state.held(), mask.size())) return rc;
        }
        for (int j = 0; j < count; j++) {
            const int32_t i = ids_host[j];
            if (i < 0 || i >= n || mask[(size_t)i]) return fail(c, S2D_E_INVALID, "s2d_grow: ids[%d] = %d is out of range, repeated or alive", j, i);
            mask[(size_t)i] = 1;
        }
    }
    if (int rc = seed_state_refused(c, cfg)) return rc;
    if (int rc = use_device(c)) return rc;
    int alive = 0;
    S2D_HIP(c, c->state.alive_count(&alive));
    const int dead = n - alive, want = ids_host ? count : std::min(count, dead);
    if (want == 0) return S2D_OK;
    SeedMap map;
    uint64_t total = 0;
    if (int rc = seed_map(c, cfg, &map, &total)) return rc;
    if (total == 0) return S2D_OK; // nowhere to draw from: nothing changes
    DevBuf<int32_t> d_ids;
    IdleAtExit idle{c->stream}; // (d_ids and the host arrays are read by the stream until the function is left)
    S2D_HIP(c, d_ids.alloc((size_t)want));
    uint8_t* flags = nullptr;
    S2D_HIP(c, c->state.begin_alive(&flags, c->d_scan_temp));
    if (ids_host) {
        S2D_HIP(c, hipMemcpyAsync(d_ids, ids_host, (size_t)want * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        S2D_HIP(c, hipMemcpyAsync(flags, mask.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    } else { // the dead rows of lowest index, chosen on the device from a scan over the dead flags
        uint32_t* work = c->state.alive_scan_work();
        S2D_HIP(c, hipMemsetAsync(d_ids, 0, (size_t)want * sizeof(int32_t), c->stream)); // (every entry a row of the context, whatever follows)
        S2D_HIP(c, launch_alive_flags(flags, 1, n, nullptr, work, nullptr, c->stream));
        S2D_HIP(c, exclusive_scan_u32(work, work, n, c->d_scan_temp, nullptr, c->stream));
        S2D_HIP(c, launch_alive_pick_dead(flags, work, n, (uint32_t)want, d_ids, c->stream));
    }
    if (int rc = seed_place(c, cfg, map, total, d_ids, want)) return rc;
    S2D_HIP(c, c->state.finish_alive(c->d_grads, c->d_scan_temp));
    alive_set_changed(c);
    c->state.alive_count_is(alive + want);
    if (grown) *grown = want;
    return S2D_OK;
}

} // extern "C"
