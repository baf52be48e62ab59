// s2d_api_weights.hip -- the pixel-weight plane through the C ABI (include/splat2d_weights.h): the two
// setters, the getter and the weighted terms.  The plane is state of the context (PixelWeights, s2d_loss_weighted.h) that the
// loss passes read (queue_loss, s2d_api_loss.hip); setting, replacing or removing it is one event, weights_replaced()
// (s2d_sequence.h).  Everything a call refuses for the context it refuses before any device work; the verdict on the plane's
// values is the check kernel's, and a plane that fails it never becomes the context's.
#include "s2d_ctx.h"

#include "../../include/splat2d_weights.h"

namespace {

int weights_alloc(s2d_ctx* c, hipError_t e)
{
    if (e == hipSuccess) return S2D_OK;
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return fail(c, S2D_E_NOMEM, "no device memory for the pixel weights");
    return fail(c, S2D_E_HIP, "setting the pixel weights failed: %s", hipGetErrorString(e));
}

void remove_plane(s2d_ctx* c)
{
    if (!c->weights.set()) return; // nothing to do without one
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream); // (a queued loss pass may still read the plane)
    c->weights.clear();
    weights_replaced(c);
}

// The candidate plane from `src` (host or device memory), checked; adopted only if every value is a weight and one is > 0.
int set_plane(s2d_ctx* c, const float* src, hipMemcpyKind kind, const char* who)
{
    if (int rc = weights_refused_by_context(c, who)) return rc;
    if (int rc = use_device(c)) return rc;
    const size_t pixels = slab_pixels(c);
    float* plane = nullptr;
    double *partial = nullptr, *out2 = nullptr;
    if (int rc = weights_alloc(c, c->weights.candidate(pixels, &plane, &partial, &out2))) return rc;
    double verdict[2] = {0.0, 0.0};
    hipError_t e = hipMemcpyAsync(plane, src, pixels * sizeof(float), kind, c->stream);
    if (e == hipSuccess) e = launch_weight_check(plane, pixels, partial, out2, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(verdict, out2, sizeof(verdict), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->weights.discard_candidate();
        return weights_alloc(c, e);
    }
    if (verdict[1] != 0.0 || !(verdict[0] > 0.0)) {
        c->weights.discard_candidate();
        if (verdict[1] != 0.0)
            return fail(c, S2D_E_INVALID, "%s: %.0f value(s) of the plane are NaN, infinite or negative; the previous plane stays", who, verdict[1]);
        return fail(c, S2D_E_INVALID, "%s: every weight is zero, nothing would train; the previous plane stays", who);
    }
    if (int rc = weights_alloc(c, c->weights.adopt(c->g.W, c->g.H, verdict[0], c->stream))) return rc;
    weights_replaced(c);
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_set_pixel_weights(s2d_ctx* c, const float* host_plane)
{
    if (!c) return S2D_E_INVALID;
    if (!host_plane) {
        remove_plane(c);
        return S2D_OK;
    }
    return set_plane(c, host_plane, hipMemcpyHostToDevice, "s2d_set_pixel_weights");
}

int s2d_set_pixel_weights_device(s2d_ctx* c, const float* device_plane)
{
    if (!c) return S2D_E_INVALID;
    if (!device_plane) {
        remove_plane(c);
        return S2D_OK;
    }
    if ((uintptr_t)device_plane & 15u) return fail(c, S2D_E_INVALID, "s2d_set_pixel_weights_device: the plane must be 16-byte aligned");
    return set_plane(c, device_plane, hipMemcpyDeviceToDevice, "s2d_set_pixel_weights_device");
}

int s2d_get_pixel_weights(s2d_ctx* c, int32_t* set, double* weight_sum, float* host_plane_or_NULL)
{
    if (!c || !set) return S2D_E_INVALID;
    *set = c->weights.set() ? 1 : 0;
    if (weight_sum) *weight_sum = c->weights.sum();
    if (!c->weights.set() || !host_plane_or_NULL) return S2D_OK;
    if (int rc = use_device(c)) return rc;
    return read_back(c, host_plane_or_NULL, c->weights.plane(), slab_pixels(c) * sizeof(float));
}

int s2d_weighted_loss_get(s2d_ctx* c, s2d_weighted_terms* out)
{
    if (!c || !out) return S2D_E_INVALID;
    if (out->struct_size != sizeof(s2d_weighted_terms)) return fail(c, S2D_E_INVALID, "s2d_weighted_terms: wrong struct_size");
    if (!c->weights.set()) return fail(c, S2D_E_INVALID, "s2d_weighted_loss_get: no pixel weights are set (s2d_set_pixel_weights)");
    if (c->loss.last_slot() < 0) return fail(c, S2D_E_STATE, "no loss pass has run under the current pixel weights");
    if (int rc = use_device(c)) return rc;
    double sums4[kWeightedTerms];
    if (int rc = read_back(c, sums4, c->weights.ring.slot(c->loss.last_slot()), sizeof(sums4))) return rc;
    double wmse = 0.0;
    const s2d_loss_terms t = loss_terms_of(c, kWeightedTerms, sums4, c->loss.last_weights(), &wmse);
    out->reserved = 0;
    out->weight_sum = c->weights.sum();
    out->mse = wmse; out->l1 = t.l1; out->dssim = t.dssim; out->total = t.total;
    return S2D_OK;
}

} // extern "C"
