// s2d_api_backdrop.hip -- a backdrop behind the splats through the C ABI (include/splat2d_backdrop.h):
// the two setters, the getter, the throughput plane and the gradient of the backdrop.  A backdrop is state of the context
// (BackdropState, s2d_backdrop.h) that the forward launch reads (raster_args, s2d_sequence.hip); setting, replacing or removing it
// is one event, backdrop_replaced() (s2d_sequence.h).  Everything a call refuses it refuses before any device work.
#include "s2d_ctx.h"

#include "../../include/splat2d_backdrop.h"

#include <cmath>

namespace {

// What the setters (`who`) refuse for the context (S2D_E_INVALID).  The configuration is asked, not the owners: the answer
// stands before anything of the context was allocated.
int backdrop_context_refused(s2d_ctx* c, const char* who)
{
    const uint32_t f = c->cfg.flags;
    if (f & S2D_CFG_COVERAGE) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_COVERAGE", who);
    if (f & S2D_CFG_COUNT_PAIRS) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_COUNT_PAIRS", who);
    if (f & S2D_CFG_EXACT_EXP) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_EXACT_EXP", who);
    if (f & S2D_CFG_REFERENCE_ORDER) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_REFERENCE_ORDER", who);
    if (c->g.row_begin != 0 || c->g.row_end != c->g.H) return fail(c, S2D_E_INVALID, "%s: the whole image is needed, this context owns a row slab", who);
    if (c->state.kind() == SplatState::Subset::Slab)
        return fail(c, S2D_E_INVALID, "%s: every splat is needed, this context holds a subset (s2d_halo_commit)", who);
    return S2D_OK;
}

int backdrop_alloc(s2d_ctx* c, hipError_t e)
{
    if (e == hipSuccess) return S2D_OK;
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return fail(c, S2D_E_NOMEM, "no device memory for the backdrop");
    return fail(c, S2D_E_HIP, "setting the backdrop failed: %s", hipGetErrorString(e));
}

// What s2d_throughput_device and s2d_backdrop_grads (`who`) need of the order of calls.
int throughput_refused(s2d_ctx* c, const char* who)
{
    if (!c->backdrop.set()) return fail(c, S2D_E_INVALID, "%s: no backdrop is set (a black one, s2d_set_backdrop, asks for the throughput alone)", who);
    if (!c->fresh.forward()) return fail(c, S2D_E_STATE, "%s: needs s2d_forward on the current parameters and backdrop", who);
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_set_backdrop(s2d_ctx* c, const float rgb[3])
{
    if (!c) return S2D_E_INVALID;
    if (!rgb) { // remove a backdrop of either kind (nothing to do without one)
        if (c->backdrop.set()) {
            c->backdrop.clear();
            backdrop_replaced(c);
        }
        return S2D_OK;
    }
    if (int rc = backdrop_context_refused(c, "s2d_set_backdrop")) return rc;
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(rgb[k])) return fail(c, S2D_E_INVALID, "s2d_set_backdrop: the colour must be finite");
    if (int rc = use_device(c)) return rc;
    if (int rc = backdrop_alloc(c, c->backdrop.set_constant(rgb, slab_pixels(c)))) return rc;
    backdrop_replaced(c);
    return S2D_OK;
}

int s2d_set_backdrop_device(s2d_ctx* c, const float* rgba32f_rows_device)
{
    if (!c) return S2D_E_INVALID;
    if (!rgba32f_rows_device) return fail(c, S2D_E_INVALID, "s2d_set_backdrop_device: NULL plane (s2d_set_backdrop(ctx, NULL) removes a backdrop)");
    if ((uintptr_t)rgba32f_rows_device & 15u) return fail(c, S2D_E_INVALID, "s2d_set_backdrop_device: the plane must be 16-byte aligned");
    if (int rc = backdrop_context_refused(c, "s2d_set_backdrop_device")) return rc;
    if (int rc = use_device(c)) return rc;
    if (int rc = backdrop_alloc(c, c->backdrop.set_plane(rgba32f_rows_device, slab_pixels(c), c->stream))) return rc;
    backdrop_replaced(c);
    return S2D_OK;
}

int s2d_get_backdrop(s2d_ctx* c, int* kind, float rgb[3])
{
    if (!c || !kind) return S2D_E_INVALID;
    *kind = (int)c->backdrop.kind();
    for (int k = 0; rgb && k < 3; k++) rgb[k] = c->backdrop.kind() == BackdropState::Constant ? c->backdrop.rgb()[k] : 0.0f;
    return S2D_OK;
}

int s2d_throughput_device(s2d_ctx* c, float* plane_device)
{
    if (!c) return S2D_E_INVALID;
    if (!plane_device) return fail(c, S2D_E_INVALID, "s2d_throughput_device: NULL output");
    if (int rc = throughput_refused(c, "s2d_throughput_device")) return rc;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, hipMemcpyAsync(plane_device, c->backdrop.throughput(), slab_pixels(c) * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return S2D_OK;
}

int s2d_backdrop_grads(s2d_ctx* c, const float* upstream_rows_device, float* dplane_device, double rgb_out[3])
{
    if (!c) return S2D_E_INVALID;
    if (((uintptr_t)upstream_rows_device | (uintptr_t)dplane_device) & 15u)
        return fail(c, S2D_E_INVALID, "s2d_backdrop_grads: the image gradient and the plane's gradient must be 16-byte aligned");
    if (!upstream_rows_device)
        if (int rc = weights_refused(c, "s2d_backdrop_grads", "a NULL upstream is image0 - target without the plane")) return rc;
    if (int rc = throughput_refused(c, "s2d_backdrop_grads")) return rc;
    if (!upstream_rows_device && !c->fresh.target()) return fail(c, S2D_E_STATE, "s2d_backdrop_grads: no target image set (s2d_set_target)");
    if (!dplane_device && !rgb_out) return S2D_OK; // nothing is asked for
    if (int rc = use_device(c)) return rc;
    BackdropGradArgs a;
    a.throughput = c->backdrop.throughput();
    a.image0 = c->d_image0; a.image_ref = c->d_ref; a.half_images = c->half_images;
    a.upstream = reinterpret_cast<const float4*>(upstream_rows_device);
    a.pixels = slab_pixels(c);
    a.dplane = reinterpret_cast<float4*>(dplane_device);
    if (rgb_out)
        if (int rc = backdrop_alloc(c, c->backdrop.sums(&a.partials, &a.sums))) return rc;
    S2D_HIP(c, launch_backdrop_grads(a, c->stream));
    if (rgb_out) return read_back(c, rgb_out, a.sums, 3 * sizeof(double));
    return S2D_OK;
}

} // extern "C"
