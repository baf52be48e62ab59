// s2d_api_loss.hip -- the loss passes of the C ABI (s2d_loss_*, s2d_step_loss; the kernels are s2d_loss.hip's).
#include "s2d_ctx.h"

#include <cmath>

namespace {

// Everything s2d_loss_* refuses for the configuration or the context, before any device work.
int loss_refused(s2d_ctx* c, const s2d_loss_config* cfg)
{
    if (!cfg || cfg->struct_size != sizeof(s2d_loss_config)) return fail(c, S2D_E_INVALID, "s2d_loss_config: NULL or wrong struct_size");
    const float w[3] = {cfg->w_mse, cfg->w_l1, cfg->w_dssim};
    for (float v : w)
        if (!(v >= 0.0f) || std::isinf(v)) return fail(c, S2D_E_INVALID, "loss weights must be finite and >= 0");
    if (w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f) return fail(c, S2D_E_INVALID, "all loss weights are zero");
    if (int rc = whole_scene_refused(c, "the loss passes", true)) return rc; // (the window crosses slab rows)
    if (c->cfg.flags & S2D_CFG_COUNT_PAIRS)
        return fail(c, S2D_E_INVALID, "pair counting (S2D_CFG_COUNT_PAIRS) has no backward pass from an image gradient");
    return coverage_refused(c, "the loss passes"); // (the native losses have no coverage term)
}

// The loss kernels of the current frame: dL/d(image0) -> dimage, the totals -> `slot` of the loss ring, the squared error
// also -> sqerr_out (the iteration's slot of the squared-error ring, or null).
int queue_loss(s2d_ctx* c, const s2d_loss_config* cfg, float4* dimage, int slot, double* sqerr_out)
{
    if (!c->fresh.forward()) return fail(c, S2D_E_STATE, "the loss needs s2d_forward on the current parameters");
    S2D_HIP(c, c->loss.ring.ensure(c->g.W, c->g.H, c->stream));
    if (cfg->w_dssim > 0.0f && !c->d_loss_maps) S2D_HIP(c, c->d_loss_maps.alloc((size_t)kLossMapPlanes * slab_pixels(c)));
    LossArgs a;
    a.image0 = c->d_image0; a.image_ref = c->d_ref; a.half_images = c->half_images; a.W = c->g.W; a.H = c->g.H;
    a.w_mse = cfg->w_mse; a.w_l1 = cfg->w_l1; a.w_dssim = cfg->w_dssim;
    a.maps = c->d_loss_maps; a.dimage = dimage; a.partial = c->loss.ring.partial(); a.out3 = c->loss.ring.slot(slot); a.sqerr_out = sqerr_out;
    a.status = c->d_status; a.iteration = c->iterations;
    if (c->weights.set()) { // L_omega: the weighted kernels, their four totals beside the three (include/splat2d_weights.h)
        WeightedLossArgs wa;
        wa.base = a;
        wa.omega = c->weights.plane(); wa.partial4 = c->weights.ring.partial(); wa.out4 = c->weights.ring.slot(slot);
        S2D_HIP(c, launch_loss_weighted(wa, c->stream));
    } else {
        S2D_HIP(c, launch_loss(a, c->stream));
    }
    c->loss.record(slot, cfg->w_mse, cfg->w_l1, cfg->w_dssim);
    return S2D_OK;
}

} // namespace

// s2d_backward / s2d_forward_backward / s2d_step under a weight plane: the weighted loss pass of the squared error alone.
int queue_weighted_backward(s2d_ctx* c, bool need_opacity_grad, bool density)
{
    static const s2d_loss_config mse_only = {(uint32_t)sizeof(s2d_loss_config), 1.0f, 0.0f, 0.0f};
    if (int rc = weights_refused_by_context(c, "the backward pass")) return rc;
    return queue_loss_backward(c, &mse_only, need_opacity_grad, density);
}

// What the weighted loss passes cannot work on (`who`): what the loss passes refuse for the context.  The setters ask this
// before they take a plane; a pass asks again, because a held set (s2d_halo_commit) may have come since.
int weights_refused_by_context(s2d_ctx* c, const char* who)
{
    if (c->cfg.flags & S2D_CFG_COVERAGE) return fail(c, S2D_E_INVALID, "%s: pixel weights are not available with S2D_CFG_COVERAGE", who);
    if (c->cfg.flags & S2D_CFG_COUNT_PAIRS) return fail(c, S2D_E_INVALID, "%s: pixel weights are not available with S2D_CFG_COUNT_PAIRS", who);
    if (c->g.row_begin != 0 || c->g.row_end != c->g.H)
        return fail(c, S2D_E_INVALID, "%s: pixel weights need the whole image, this context owns a row slab", who);
    if (c->state.kind() == SplatState::Subset::Slab)
        return fail(c, S2D_E_INVALID, "%s: pixel weights need every splat, this context holds a subset (s2d_halo_commit); "
                    "s2d_set_pixel_weights(ctx, NULL) removes them", who);
    return S2D_OK;
}

// s2d_backward for the loss: the loss kernels into the context's gradient image, the backward walk from it, and the
// squared error of the iteration in the ring as the loss finalize left it (SqerrBy::LossPass).
int queue_loss_backward(s2d_ctx* c, const s2d_loss_config* cfg, bool need_opacity_grad, bool density)
{
    if (!c->fresh.forward()) return fail(c, S2D_E_STATE, "the backward pass needs s2d_forward on the current parameters");
    if (!c->d_loss_grad) S2D_HIP(c, c->d_loss_grad.alloc(slab_pixels(c)));
    if (int rc = queue_loss(c, cfg, c->d_loss_grad, TermRing::slot_of(c->iterations), c->trace.job(c->iterations).out)) return rc;
    if (int rc = queue_backward(c, need_opacity_grad, c->d_loss_grad, density)) return rc;
    return backward_queued(c, SqerrBy::LossPass);
}

// The `terms` sums of a loss pass (kLossTerms, or kWeightedTerms under a plane) -> the means and the total; a term with
// weight 0 was not formed.  sums[0] is the squared error on the 255 scale, which t.mse reports; the last three of either are
// the squared error the total counts (without a plane sums[0] once more, under one omega * it), the sum of |d| and that of 1 - s.
s2d_loss_terms loss_terms_of(const s2d_ctx* c, int terms, const double* sums, const float* w, double* weighted_mse)
{
    const double* last = sums + terms - 3;
    const double n3 = mse_norm(c);
    s2d_loss_terms t;
    t.mse = sums[0] / (255.0 * 255.0) / n3;
    const double wmse = last[0] / (255.0 * 255.0) / n3;
    t.l1 = w[1] > 0.0f ? last[1] / n3 : std::nan("");
    t.dssim = w[2] > 0.0f ? last[2] / n3 : std::nan("");
    t.total = 0.0;
    if (w[0] > 0.0f) t.total += (double)w[0] * 0.5 * wmse;
    if (w[1] > 0.0f) t.total += (double)w[1] * t.l1;
    if (w[2] > 0.0f) t.total += (double)w[2] * t.dssim;
    if (weighted_mse) *weighted_mse = wmse;
    return t;
}

// The ring the loss passes of the context write now: the four totals under a plane, the three without.
const TermRing& current_ring(const s2d_ctx* c) { return c->weights.set() ? c->weights.ring : c->loss.ring; }

extern "C" {

int s2d_loss_image_grads_device(s2d_ctx* c, const s2d_loss_config* cfg, float* dimage_rows_device)
{
    if (!c || !dimage_rows_device) return S2D_E_INVALID;
    if (int rc = loss_refused(c, cfg)) return rc;
    if ((uintptr_t)dimage_rows_device & 15u) return fail(c, S2D_E_INVALID, "the image gradient must be 16-byte aligned");
    if (int rc = use_device(c)) return rc;
    return queue_loss(c, cfg, reinterpret_cast<float4*>(dimage_rows_device), TermRing::kEvalSlot, nullptr);
}

int s2d_loss_backward(s2d_ctx* c, const s2d_loss_config* cfg, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = loss_refused(c, cfg)) return rc;
    WalkFlags wf;
    if (int rc = parse_walk_flags(c, flags, false, &wf)) return rc;
    if (int rc = use_device(c)) return rc;
    return queue_loss_backward(c, cfg, wf.need_opacity_grad, wf.density);
}

int s2d_loss_get(s2d_ctx* c, s2d_loss_terms* out)
{
    if (!c || !out) return S2D_E_INVALID;
    if (c->loss.last_slot() < 0) return fail(c, S2D_E_STATE, "no loss pass has run yet");
    if (int rc = use_device(c)) return rc;
    const TermRing& ring = current_ring(c); // (a pass older than the plane is forgotten when the plane is set: the last one was a weighted one)
    double sums[kWeightedTerms];
    if (int rc = read_back(c, sums, ring.slot(c->loss.last_slot()), (size_t)ring.terms() * sizeof(double))) return rc;
    *out = loss_terms_of(c, ring.terms(), sums, c->loss.last_weights());
    return S2D_OK;
}

int s2d_step_loss(s2d_ctx* c, int32_t iters, uint32_t flags, const s2d_loss_config* cfg, double* loss_out, double* mse_out)
{
    if (!c || iters < 0) return S2D_E_INVALID;
    if (int rc = loss_refused(c, cfg)) return rc;
    return run_steps(c, iters, flags, cfg, loss_out, mse_out);
}

} // extern "C"
