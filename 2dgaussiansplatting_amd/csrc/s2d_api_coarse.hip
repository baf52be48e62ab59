// s2d_api_coarse.hip -- coarse-to-fine fitting through the C ABI (include/splat2d_coarse.h):
// s2d_view_target_device, the context's target resampled to a view's window, and s2d_step_view, whole iterations at a view's
// size.  An iteration is s2d_view_backward_device(S2D_VIEW_BWD_FROM_TARGET) with view_fit_kernel (s2d_view_fit.hip) in the place of
// view_gradient_kernel, the sum of the tile errors it leaves, and queue_adam (s2d_sequence.h) -- so everything an Adam step is
// an event for happens as it does for s2d_adam_step.  Like every view it goes through no other event: image0, the training
// lists, the squared-error ring of the training image and the density statistics are not touched.  The library's own target is
// derived state of the view's scratch: target_replaced() (s2d_sequence.hip) makes it stale.
#include "s2d_ctx.h"
#include "s2d_view_target_math.h"

#include "../../include/splat2d_coarse.h"

#include <algorithm>
#include <cmath>

namespace {

ViewWindow window_of(const s2d_view_config* cfg)
{
    ViewWindow w;
    w.out_width = cfg->out_width, w.out_height = cfg->out_height;
    w.origin_x = cfg->origin_x, w.origin_y = cfg->origin_y, w.zoom = cfg->zoom;
    return w;
}

// The window of the context's target into `out` (queued).
int resample_target(s2d_ctx* c, const s2d_view_config* cfg, float4* out)
{
    S2D_HIP(c, launch_view_target(c->d_ref, c->half_images, c->g.W, c->g.H, cfg->origin_x, cfg->origin_y, cfg->zoom, cfg->out_width,
                                  cfg->out_height, out, c->stream));
    return S2D_OK;
}

// The library's own target of the configuration, rebuilt (queued) unless it holds this window of the current target.
int own_target(s2d_ctx* c, const s2d_view_config* cfg, const float4** out)
{
    float4* t = nullptr;
    bool current = false;
    if (int rc = view_alloc(c, c->view.own_target(window_of(cfg), c->stream, &t, &current), "the target")) return rc;
    if (!current) {
        if (int rc = resample_target(c, cfg, t)) return rc;
        c->view.own_target_built();
    }
    *out = t;
    return S2D_OK;
}

// One iteration but for its Adam step (queued behind the list build): the view's lists, view_fit_kernel with deterministic mode's
// gather, the sum of the tile errors into slot `ring_slot` of the ring (*ring: its first slot), the adjoint of the record
// transform into the gradient buffer.
int queue_view_fit(s2d_ctx* c, const s2d_view_config* cfg, const float4* target, bool need_opacity_grad, int ring_slot, double** ring)
{
    ViewGradientArgs a;
    float* record_grads = nullptr;
    if (int rc = view_backward_prepare(c, cfg, need_opacity_grad, &a.walk, &record_grads)) return rc;
    SqerrJob job{};
    if (int rc = view_alloc(c, c->view.fit_errors(a.walk.g.num_tiles, c->stream, &job, &a.walk.tile_sqerr), "the tile errors")) return rc;
    *ring = job.out;
    job.out += ring_slot;
    a.src = target; a.from_target = true;
    a.out_width = cfg->out_width; a.samples = view_samples(cfg->samples);
    S2D_HIP(c, launch_view_fit(a, c->stream));
    S2D_HIP(c, launch_sqerr_finalize(job, c->d_status, c->iterations, c->stream));
    return view_adjoint(c, cfg, record_grads);
}

// The resample walks 1 / zoom source pixels per axis in ONE lane per output pixel: below kViewTargetMinZoom it is refused.
int target_zoom_refused(s2d_ctx* c, const s2d_view_config* cfg, const char* who)
{
    if (cfg->zoom < kViewTargetMinZoom)
        return fail(c, S2D_E_INVALID, "%s: the target is not resampled below zoom 1/%d (one output pixel would cover more than %d x %d source pixels)",
                    who, (int)(1.0f / kViewTargetMinZoom), (int)(1.0f / kViewTargetMinZoom), (int)(1.0f / kViewTargetMinZoom));
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_view_target_device(s2d_ctx* c, const s2d_view_config* cfg, float* out_device)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = view_pass_config_refused(c, cfg, "s2d_view_target_device")) return rc;
    if (int rc = target_zoom_refused(c, cfg, "s2d_view_target_device")) return rc;
    if (int rc = view_pass_context_refused(c, "s2d_view_target_device")) return rc;
    if (!out_device) return fail(c, S2D_E_INVALID, "s2d_view_target_device: NULL output");
    if ((uintptr_t)out_device & 15u) return fail(c, S2D_E_INVALID, "s2d_view_target_device: the buffer must be 16-byte aligned");
    if (int rc = use_device(c)) return rc;
    return resample_target(c, cfg, reinterpret_cast<float4*>(out_device));
}

int s2d_step_view(s2d_ctx* c, const s2d_view_config* cfg, const float* target_device, int32_t iters, uint32_t flags, double* mse_out)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = view_pass_config_refused(c, cfg, "s2d_step_view")) return rc;
    if (int rc = view_pass_context_refused(c, "s2d_step_view")) return rc;
    if (int rc = weights_refused(c, "s2d_step_view", "the plane is not resampled to a view")) return rc;
    if (int rc = backdrop_refused(c, "s2d_step_view")) return rc; // (view_fit_kernel forms the final colour itself, without the backdrop)
    if (flags & ~S2D_STEP_OPTIMIZE_OPACITY) return fail(c, S2D_E_INVALID, "s2d_step_view: unknown flags %#x", flags);
    if (iters < 0) return fail(c, S2D_E_INVALID, "s2d_step_view: iters < 0");
    if ((uintptr_t)target_device & 15u) return fail(c, S2D_E_INVALID, "s2d_step_view: the target must be 16-byte aligned");
    if (!target_device)
        if (int rc = target_zoom_refused(c, cfg, "s2d_step_view")) return rc;
    if (iters == 0) return S2D_OK;
    if (int rc = use_device(c)) return rc;
    const float4* target = reinterpret_cast<const float4*>(target_device);
    if (!target)
        if (int rc = own_target(c, cfg, &target)) return rc;
    // as s2d_step (parse_walk_flags): the walk forms the opacity gradient exactly when the step uses it -- what a caller of
    // s2d_view_backward_device says with S2D_BWD_SKIP_OPACITY_GRAD
    const bool need_opacity_grad = (flags & S2D_STEP_OPTIMIZE_OPACITY) != 0;
    const double norm = (double)((long long)cfg->out_height * cfg->out_width * 3);
    const int call_first_iter = c->iterations;
    for (int done = 0; done < iters;) {
        const int piece = std::min<int>(iters - done, ViewScratch::kFitRing);
        double* ring = nullptr;
        for (int k = 0; k < piece; k++) {
            if (int rc = queue_view_fit(c, cfg, target, need_opacity_grad, k, &ring)) return rc;
            if (int rc = queue_adam(c, flags)) return rc;
        }
        if (mse_out) {
            if (int rc = read_back(c, mse_out + done, ring, (size_t)piece * sizeof(double))) return rc;
            for (int k = 0; k < piece; k++) mse_out[done + k] /= norm; // main.cpp:805
        }
        done += piece;
    }
    const int rc = check_status(c);
    if (rc == S2D_E_NONFINITE && mse_out) {
        // as s2d_step: the trace ends with the iteration whose Adam step failed; the sums of the later ones were never formed
        const int last_valid = c->h_status->first_nonfinite_iter - call_first_iter;
        for (int k = std::max(last_valid + 1, 0); k < iters; k++) mse_out[k] = std::nan("");
    }
    return rc;
}

} // extern "C"
