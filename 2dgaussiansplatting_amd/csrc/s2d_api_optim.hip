// s2d_api_optim.hip -- the optimiser controls through the C ABI: rates per parameter group with their decay
// (s2d_set_optim, s2d_optim_rates_at; the rules are s2d_optim_rates.h) and the frozen mask (s2d_set_frozen,
// s2d_set_frozen_device).  They change what adam_args() hands to the Adam launch and nothing else: no projection, no list
// and no frame is stale after any of them.
#include "s2d_ctx.h"

namespace {

// The mask from host (waits: the caller's array is read by the stream until then) or device memory (queued); null: none.
int set_frozen(s2d_ctx* c, const char* who, const uint8_t* mask, bool from_host)
{
    if (int rc = whole_scene_refused(c, who, true)) return rc;
    if (!mask) {
        c->has_frozen = false;
        return S2D_OK;
    }
    if (int rc = use_device(c)) return rc;
    if (c->d_frozen.capacity() < (size_t)c->n || !c->d_frozen) {
        S2D_HIP(c, hipStreamSynchronize(c->stream)); // (a launch still reading the old mask)
        S2D_HIP(c, c->d_frozen.alloc((size_t)c->n));
    }
    if (c->n > 0)
        S2D_HIP(c, hipMemcpyAsync(c->d_frozen, mask, (size_t)c->n, from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    c->has_frozen = true;
    if (from_host) S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_set_optim(s2d_ctx* c, const s2d_optim_config* cfg)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = whole_scene_refused(c, "s2d_set_optim", true)) return rc;
    if (!cfg) {
        c->has_optim = false;
        return S2D_OK;
    }
    if (const char* why = optim_config_refused(cfg)) return fail(c, S2D_E_INVALID, "s2d_optim_config: %s", why);
    c->optim = *cfg;
    c->has_optim = true;
    return S2D_OK;
}

int s2d_optim_rates_at(s2d_ctx* c, int32_t iteration, float rates[5])
{
    if (!c || !rates) return S2D_E_INVALID;
    if (int rc = whole_scene_refused(c, "s2d_optim_rates_at", true)) return rc;
    if (iteration < 0) return fail(c, S2D_E_INVALID, "s2d_optim_rates_at: iteration %d < 0", iteration);
    optim_rates_at(c->has_optim ? &c->optim : nullptr, c->lr, iteration, rates);
    return S2D_OK;
}

int s2d_set_frozen(s2d_ctx* c, const uint8_t* frozen_host)
{
    if (!c) return S2D_E_INVALID;
    return set_frozen(c, "s2d_set_frozen", frozen_host, true);
}

int s2d_set_frozen_device(s2d_ctx* c, const uint8_t* frozen_device)
{
    if (!c) return S2D_E_INVALID;
    return set_frozen(c, "s2d_set_frozen_device", frozen_device, false);
}

} // extern "C"
