// s2d_api_view.hip -- view rendering through the C ABI (s2d_view_splats, s2d_render_view, s2d_render_view_device,
// s2d_view_release; s2d_view.h).  A view reads the context's current splats and writes the caller's
// buffer and the ViewScratch of the context; it goes through none of the events of s2d_sequence.h, because nothing that
// training derived becomes stale: image0, the tile lists and their rebuild counters, the projection, the hand-over, the
// status word, the squared-error ring and the density statistics are not touched.
// The backward pass through a view (s2d_view_backward_device, s2d_view_grads) is as read-only, but for the
// gradient buffer it adds into -- which no event of s2d_sequence.h watches either: s2d_backward_image_grads accumulates the same way.
#include "s2d_ctx.h"

#include "../../include/splat2d_test.h"

// (view_alloc, view_lists, the two view_pass_*_refused, view_backward_prepare and view_adjoint are shared with
// s2d_api_coarse.hip: s2d_ctx.h)
// A failed allocation of the view's scratch: S2D_E_NOMEM when the device is out of memory, S2D_E_HIP otherwise.
int view_alloc(s2d_ctx* c, hipError_t e, const char* what)
{
    if (e == hipSuccess) return S2D_OK;
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return fail(c, S2D_E_NOMEM, "no device memory for %s of the view", what);
    return fail(c, S2D_E_HIP, "allocating %s of the view failed: %s", what, hipGetErrorString(e));
}

namespace {

// Everything the view calls (`who`) refuse for the configuration or the context, before any device work (S2D_E_INVALID).
// draws: the call rasterises the view (a plane backdrop has no view kernel).
int view_refused(s2d_ctx* c, const s2d_view_config* cfg, const char* who, bool draws = false)
{
    if (!cfg) return fail(c, S2D_E_INVALID, "%s: NULL s2d_view_config", who);
    if (const char* why = view_config_invalid(cfg->struct_size, (uint32_t)sizeof(s2d_view_config), cfg->out_width, cfg->out_height,
                                              cfg->origin_x, cfg->origin_y, cfg->zoom, cfg->filter_var, cfg->samples, cfg->format,
                                              S2D_VIEW_RGBA8))
        return fail(c, S2D_E_INVALID, "%s: s2d_view_config: %s", who, why);
    if (draws && c->backdrop.kind() == BackdropState::Plane)
        return fail(c, S2D_E_INVALID, "%s: a view over a plane backdrop is not available (the plane would have to be resampled)", who);
    return whole_scene_refused(c, who, true); // (an alive set and reference order are no obstacle)
}

// The n x 9 records of the view into the scratch (queued).
int view_records(s2d_ctx* c, const s2d_view_config* cfg, float** rows)
{
    if (int rc = view_alloc(c, c->view.rows((size_t)c->n, rows), "the records")) return rc;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, launch_view_transform(now.splats, c->n, view_xform(cfg->origin_x, cfg->origin_y, cfg->zoom, cfg->filter_var, cfg->samples),
                                     *rows, c->stream));
    return S2D_OK;
}

// What a pass over the view's lists as they stand works on: lists, records, hand-over and slots, the grid and the kernel variant.
void view_walk(s2d_ctx* c, const s2d_view_config* cfg, RasterArgs* a)
{
    c->view.surface().fill(a, 0, c->n);
    a->g = view_geometry(cfg->out_width, cfg->out_height, view_samples(cfg->samples));
    a->exact_exp = (c->cfg.flags & S2D_CFG_EXACT_EXP) != 0;
}

// The raster kernel over the view's lists as they stand (queued).
int view_raster(s2d_ctx* c, const s2d_view_config* cfg, void* out)
{
    ViewRasterArgs a;
    view_walk(c, cfg, &a.walk);
    a.out = out; a.out_width = cfg->out_width; a.samples = view_samples(cfg->samples); a.rgba8 = cfg->format == S2D_VIEW_RGBA8;
    if (c->backdrop.set()) { // (a constant: view_refused) the composite per sample, backdrop_view_kernel
        for (int k = 0; k < 3; k++) a.rgb[k] = c->backdrop.rgb()[k];
        S2D_HIP(c, launch_backdrop_view(a, c->stream));
        return S2D_OK;
    }
    a.walk.coverage = coverage(c);
    S2D_HIP(c, launch_view_raster(a, c->stream));
    return S2D_OK;
}

} // namespace

// The records, the projection and the lists of the view.  Queued, but for the one wait of a list build (the pair count) and
// for the waits of buffers that are replaced.
int view_lists(s2d_ctx* c, const s2d_view_config* cfg)
{
    const Geometry g = view_geometry(cfg->out_width, cfg->out_height, view_samples(cfg->samples));
    RasterSurface& surface = c->view.surface();
    const PairScratch::Mode mode = c->surface.deterministic() ? PairScratch::Mode::Deterministic : PairScratch::Mode::Atomic; // (a view has no reference-order pass)
    if (!surface.on(g))
        if (int rc = view_alloc(c, surface.create(g, (size_t)c->n, (c->cfg.flags & S2D_CFG_GENERIC_BINNING) != 0, mode, c->stream), "the lists")) return rc;
    float* rows = nullptr;
    if (int rc = view_records(c, cfg, &rows)) return rc;
    S2D_HIP(c, launch_project(surface.project_args(rows, c->state.held(), c->n, 0.0f), c->stream)); // the exact rectangles; a dead row gets an empty one
    uint64_t total = 0;
    S2D_HIP(c, surface.count(0, c->n, c->d_scan_temp, &total));
    if (total > c->ranges.budget() || total >= kMaxPairs)
        return fail(c, S2D_E_NOMEM, "the view needs %llu (tile, splat) pairs, S2D_CHUNK_PAIRS allows %llu (views are not rendered by index ranges)",
                    (unsigned long long)total, (unsigned long long)c->ranges.budget());
    if (int rc = view_alloc(c, surface.ensure_pairs(total, false), "the (tile, splat) pairs")) return rc;
    S2D_HIP(c, surface.finish());
    return S2D_OK;
}

// What the passes with a backward walk through a view (`who`) refuse, before any device work (S2D_E_INVALID): for the
// configuration, and for the context.
int view_pass_config_refused(s2d_ctx* c, const s2d_view_config* cfg, const char* who)
{
    if (int rc = view_refused(c, cfg, who)) return rc;
    if (cfg->format != S2D_VIEW_RGBA32F) return fail(c, S2D_E_INVALID, "%s: the gradient of a view is RGBA32F (format S2D_VIEW_RGBA32F)", who);
    return S2D_OK;
}

int view_pass_context_refused(s2d_ctx* c, const char* who)
{
    if (c->cfg.flags & S2D_CFG_COUNT_PAIRS) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_COUNT_PAIRS", who);
    if (c->surface.reference_order()) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_REFERENCE_ORDER", who);
    return coverage_refused(c, who); // (the view gradient kernels carry no coverage)
}

// What every pass with a backward walk through a view starts with (queued behind the list build): records, projection, lists,
// the zeroed n x 9 gradients of the view's records (*grads), the raster scratch of the lists, and `walk` filled for the launch.
int view_backward_prepare(s2d_ctx* c, const s2d_view_config* cfg, bool need_opacity_grad, RasterArgs* walk, float** grads)
{
    if (int rc = view_lists(c, cfg)) return rc;
    RasterSurface& surface = c->view.surface();
    if (int rc = view_alloc(c, c->view.grads((size_t)c->n, c->stream, grads), "the gradient pass")) return rc;
    if (int rc = view_alloc(c, surface.ensure_pairs(surface.lists().capacity(), true), "the gradient pass")) return rc; // the scratch, first time on these lists
    view_walk(c, cfg, walk);
    walk->grads = *grads;
    walk->need_opacity_grad = need_opacity_grad;
    surface.backward_walk(walk);
    return S2D_OK;
}

// The gradients of the view's records, taken back through the record transform, ADDED into the context's gradient buffer (queued).
int view_adjoint(s2d_ctx* c, const s2d_view_config* cfg, const float* record_grads)
{
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, launch_view_adjoint(now.splats, c->state.held(), c->n,
                                   view_xform(cfg->origin_x, cfg->origin_y, cfg->zoom, cfg->filter_var, cfg->samples), record_grads,
                                   c->d_grads, c->stream));
    return S2D_OK;
}

namespace {

// The whole view into `out` (device memory): records, projection, lists, raster.
int view_render(s2d_ctx* c, const s2d_view_config* cfg, void* out)
{
    if (int rc = view_lists(c, cfg)) return rc;
    return view_raster(c, cfg, out);
}

// Everything the gradient calls (`who`) refuse, before any device work (S2D_E_INVALID).
int view_gradient_refused(s2d_ctx* c, const s2d_view_config* cfg, const float* src, uint32_t flags, const char* who)
{
    if (int rc = view_pass_config_refused(c, cfg, who)) return rc;
    if (!src) return fail(c, S2D_E_INVALID, "%s: NULL image gradient (or target)", who);
    if ((uintptr_t)src & 15u) return fail(c, S2D_E_INVALID, "%s: the image gradient (or target) must be 16-byte aligned", who);
    if (flags & ~(S2D_VIEW_BWD_FROM_TARGET | S2D_BWD_SKIP_OPACITY_GRAD)) return fail(c, S2D_E_INVALID, "%s: unknown flags %#x", who, flags);
    if (flags & S2D_VIEW_BWD_FROM_TARGET)
        if (int rc = weights_refused(c, who, "S2D_VIEW_BWD_FROM_TARGET forms view - target without the plane, which is not resampled to a view")) return rc;
    if (int rc = backdrop_refused(c, who)) return rc; // (view_gradient_kernel forms the final colour itself, without the backdrop)
    return view_pass_context_refused(c, who);
}

// The gradients of the view's records from `src` (dL/d(view), or the target with S2D_VIEW_BWD_FROM_TARGET) into the scratch's
// n x 9 buffer (queued behind the list build): records, projection, lists, view_gradient_kernel, deterministic mode's gather.
int view_record_grads(s2d_ctx* c, const s2d_view_config* cfg, const float* src, uint32_t flags, float** grads)
{
    ViewGradientArgs a;
    if (int rc = view_backward_prepare(c, cfg, !(flags & S2D_BWD_SKIP_OPACITY_GRAD), &a.walk, grads)) return rc;
    a.src = reinterpret_cast<const float4*>(src);
    a.out_width = cfg->out_width; a.samples = view_samples(cfg->samples);
    a.from_target = (flags & S2D_VIEW_BWD_FROM_TARGET) != 0;
    S2D_HIP(c, launch_view_gradient(a, c->stream));
    return S2D_OK;
}

size_t view_bytes(const s2d_view_config* cfg)
{
    return (size_t)cfg->out_width * (size_t)cfg->out_height * (cfg->format == S2D_VIEW_RGBA8 ? 4u : 16u);
}

} // namespace

extern "C" {

int s2d_view_splats(s2d_ctx* c, const s2d_view_config* cfg, s2d_splat* out_host)
{
    if (!c) return S2D_E_INVALID;
    if (!out_host && c->n) return fail(c, S2D_E_INVALID, "s2d_view_splats: NULL output");
    if (int rc = view_refused(c, cfg, "s2d_view_splats")) return rc;
    if (int rc = use_device(c)) return rc;
    float* rows = nullptr;
    if (int rc = view_records(c, cfg, &rows)) return rc;
    return read_back(c, out_host, rows, (size_t)c->n * sizeof(s2d_splat));
}

int s2d_render_view_device(s2d_ctx* c, const s2d_view_config* cfg, void* out_device)
{
    if (!c) return S2D_E_INVALID;
    if (!out_device) return fail(c, S2D_E_INVALID, "s2d_render_view_device: NULL output");
    if (int rc = view_refused(c, cfg, "s2d_render_view_device", true)) return rc;
    if ((uintptr_t)out_device & (cfg->format == S2D_VIEW_RGBA8 ? 3u : 15u))
        return fail(c, S2D_E_INVALID, "s2d_render_view_device: the buffer must be 16-byte (RGBA32F) or 4-byte (RGBA8) aligned");
    if (int rc = use_device(c)) return rc;
    return view_render(c, cfg, out_device);
}

int s2d_render_view(s2d_ctx* c, const s2d_view_config* cfg, void* out_host)
{
    if (!c) return S2D_E_INVALID;
    if (!out_host) return fail(c, S2D_E_INVALID, "s2d_render_view: NULL output");
    if (int rc = view_refused(c, cfg, "s2d_render_view", true)) return rc;
    if (int rc = use_device(c)) return rc;
    void* image = nullptr;
    if (int rc = view_alloc(c, c->view.image(view_bytes(cfg), &image), "the image")) return rc;
    if (int rc = view_render(c, cfg, image)) return rc;
    return read_back(c, out_host, image, view_bytes(cfg));
}

int s2d_view_backward_device(s2d_ctx* c, const s2d_view_config* cfg, const float* dview_or_target_device, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = view_gradient_refused(c, cfg, dview_or_target_device, flags, "s2d_view_backward_device")) return rc;
    if (int rc = use_device(c)) return rc;
    float* record_grads = nullptr;
    if (int rc = view_record_grads(c, cfg, dview_or_target_device, flags, &record_grads)) return rc;
    return view_adjoint(c, cfg, record_grads);
}

int s2d_view_grads(s2d_ctx* c, const s2d_view_config* cfg, const float* dview_or_target_device, uint32_t flags, s2d_splat* dview_records_host)
{
    if (!c) return S2D_E_INVALID;
    if (!dview_records_host && c->n) return fail(c, S2D_E_INVALID, "s2d_view_grads: NULL output");
    if (int rc = view_gradient_refused(c, cfg, dview_or_target_device, flags, "s2d_view_grads")) return rc;
    if (int rc = use_device(c)) return rc;
    float* record_grads = nullptr;
    if (int rc = view_record_grads(c, cfg, dview_or_target_device, flags, &record_grads)) return rc;
    return read_back(c, dview_records_host, record_grads, (size_t)c->n * sizeof(s2d_splat));
}

// (include/splat2d_test.h) The raster kernel of the view alone, over the lists the last rendering of this configuration left.
int s2d_debug_view_raster(s2d_ctx* c, const s2d_view_config* cfg, void* out_device)
{
    if (!c || !out_device) return S2D_E_INVALID;
    if (int rc = view_refused(c, cfg, "s2d_debug_view_raster", true)) return rc;
    if ((uintptr_t)out_device & (cfg->format == S2D_VIEW_RGBA8 ? 3u : 15u)) return fail(c, S2D_E_INVALID, "s2d_debug_view_raster: misaligned buffer");
    if (!c->view.has_lists(view_geometry(cfg->out_width, cfg->out_height, view_samples(cfg->samples))))
        return fail(c, S2D_E_STATE, "s2d_debug_view_raster: no lists of this raster grid (render the view first)");
    if (int rc = use_device(c)) return rc;
    return view_raster(c, cfg, out_device);
}

int s2d_view_release(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (!c->view.allocated()) return S2D_OK;
    if (int rc = use_device(c)) return rc;
    c->view.release(c->stream);
    return S2D_OK;
}

} // extern "C"
