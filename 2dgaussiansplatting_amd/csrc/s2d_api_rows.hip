// s2d_api_rows.hip -- slab ownership through the C ABI (the kernels are s2d_halo.hip's): held sets, rows
// of the per-splat arrays, gradient exchange.  All pointers of these calls are device pointers of the caller.
#include "s2d_ctx.h"

extern "C" {

int s2d_halo_masks(s2d_ctx* c, int32_t world, const int32_t* row_bounds, float margin_rows, uint32_t* masks_device)
{
    if (!c || !row_bounds || !masks_device || world < 1 || world > 32 || !(margin_rows >= 0.0f)) return S2D_E_INVALID;
    for (int q = 0; q < world; q++)
        if (row_bounds[q] > row_bounds[q + 1]) return S2D_E_INVALID;
    if (int rc = coverage_refused(c, "s2d_halo_masks")) return rc;
    if (int rc = backdrop_refused(c, "s2d_halo_masks")) return rc;
    if (c->state.kind() == SplatState::Subset::Alive) // (its flags are no hold set: the two kinds of subset exclude each other)
        return fail(c, S2D_E_INVALID, "s2d_halo_masks: this context has an alive set (s2d_set_alive(NULL) first)");
    if (int rc = use_device(c)) return rc;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, launch_halo_masks(now.splats, c->state.held(), c->n, world, row_bounds, margin_rows, masks_device, c->stream));
    return S2D_OK;
}

int s2d_halo_commit(s2d_ctx* c, const uint32_t* masks_device, int32_t rank, int32_t added)
{
    if (!c || rank < 0 || rank > 31) return S2D_E_INVALID;
    if (int rc = coverage_refused(c, "s2d_halo_commit")) return rc;
    if (int rc = backdrop_refused(c, "s2d_halo_commit")) return rc;
    if (masks_device && c->surface.reference_order())
        return fail(c, S2D_E_INVALID, "reference order (S2D_CFG_REFERENCE_ORDER) has no slab ownership: the chains run over all splats");
    if (masks_device && (c->has_optim || c->has_frozen))
        return fail(c, S2D_E_INVALID, "slab ownership derives its hold margins from the one training_rate: clear s2d_set_optim / s2d_set_frozen first");
    if (c->state.kind() == SplatState::Subset::Alive) { // the two kinds of subset exclude each other
        if (masks_device) return fail(c, S2D_E_INVALID, "s2d_halo_commit: this context has an alive set (s2d_set_alive(NULL) first)");
        return S2D_OK; // (it holds every row it has already)
    }
    if (int rc = use_device(c)) return rc;
    const bool had = c->state.held() != nullptr;
    S2D_HIP(c, c->state.commit(masks_device, rank, c->d_scan_temp));
    held_set_changed(c, had, masks_device != nullptr, added != 0);
    return S2D_OK;
}

// The array of a row call and its row width, on the context's device: the gradients, or the state's arrays with
// everything queued so far in them.
static int rows_base(s2d_ctx* c, int32_t what, float** base, int* w)
{
    if (what != S2D_ROWS_GRADS && what != S2D_ROWS_SPLATS && what != S2D_ROWS_ADAM) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    *base = c->d_grads;
    *w = what == S2D_ROWS_ADAM ? 18 : 9;
    if (what == S2D_ROWS_GRADS) return S2D_OK;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    *base = what == S2D_ROWS_SPLATS ? now.splats : now.adams;
    return S2D_OK;
}

int s2d_rows_gather(s2d_ctx* c, int32_t what, const int32_t* ids_device, int32_t count, float* out_device)
{
    if (!c || count < 0 || (count > 0 && (!ids_device || !out_device))) return S2D_E_INVALID;
    float* base;
    int w;
    if (int rc = rows_base(c, what, &base, &w)) return rc;
    S2D_HIP(c, launch_rows_gather(base, w, ids_device, count, c->n, out_device, c->stream));
    return S2D_OK;
}

int s2d_rows_scatter(s2d_ctx* c, int32_t what, const int32_t* ids_device, int32_t count, const float* in_device)
{
    if (!c || count < 0 || (count > 0 && (!ids_device || !in_device))) return S2D_E_INVALID;
    float* base;
    int w;
    if (int rc = rows_base(c, what, &base, &w)) return rc;
    S2D_HIP(c, launch_rows_scatter(base, w, ids_device, count, c->n, in_device, c->stream));
    return rows_replaced(c, what);
}

int s2d_grads_combine(s2d_ctx* c, const int32_t* rows_device, int32_t n_rows, const int32_t* src_device, int32_t world,
                      const float* recv_device)
{
    if (!c || n_rows < 0 || world < 1 || world > 32 || (n_rows > 0 && (!rows_device || !src_device))) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, launch_grads_combine(c->d_grads, rows_device, n_rows, src_device, world, recv_device, c->n, c->stream));
    return S2D_OK;
}

} // extern "C"
