// s2d_ctx.h -- the context behind the C ABI's handle, and the few helpers every unit that takes one needs.  Internal:
// s2d_sequence.hip and the entry-point units s2d_api*.hip include it; nothing of it is exported.
#pragma once

#include "../../include/splat2d.h"

#include <cstdarg>
#include <cstdio>

#include "s2d_backdrop.h"
#include "s2d_device.h"
#include "s2d_context.h"
#include "s2d_lists.h"
#include "s2d_loss.h"
#include "s2d_loss_weighted.h"
#include "s2d_optim_rates.h"
#include "s2d_owned.h"
#include "s2d_seed.h"
#include "s2d_sequence.h"
#include "s2d_state.h"
#include "s2d_view.h"

using namespace s2d;

struct s2d_ctx {
    s2d_config cfg{};
    Geometry g{};
    int n = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    float lr = 0.05f;

    SplatState state;            // parameters, optimiser state, the held set of slab ownership or the alive set (s2d_state.h)
    DevBuf<float> d_grads_own;   // gradients (AoS, the reference's layout)
    float* d_grads = nullptr;    // buffer in use (own or bound)
    // projection + binning
    DevBuf<uint32_t> d_scan_temp;               // lent to the list builds (the views' too) and to s2d_halo_commit
    RasterSurface surface;                      // the training image's projection, rectangles, lists and raster scratch (s2d_context.h)
    IndexRanges ranges;                         // scenes beyond one set of lists: the cut, the carry, the progress of a pass
    Freshness fresh;         // which of target, frames, projection and lists are current (s2d_sequence.h)
    ListReuse reuse;         // when lists are rebuilt on schedule, and the stamped containment check (s2d_context.h)
    // images
    // image0 / imageRef (main.cpp:310, :254): the rows [row_begin, row_end) of this context's slab only -- a context
    // never touches another row, so a 1/8 slab of 8192^2 holds 2 x 134 MB instead of 2 x 1.07 GB
    DevBuf<uint8_t> d_image0;  // bytes: RGBA32F, or 4 x fp16 per pixel with S2D_CFG_FP16_IMAGES
    DevBuf<uint8_t> d_ref;
    bool half_images = false;
    size_t pixel_bytes = sizeof(float4);
    SqerrTrace trace;          // the tile errors of a backward pass and the ring of per-iteration sums (s2d_state.h)
    DensityStats density;      // what the passes with S2D_BWD_DENSITY_STATS accumulated (s2d_state.h)
    // loss passes (s2d_loss_*, s2d_loss.h): everything here is allocated by the first call that needs it
    LossTrace loss;                // per-tile sums and the ring of per-iteration totals
    DevBuf<float> d_loss_maps;     // [9][pixels]: the derivative maps between the two window passes (w_dssim > 0 only)
    DevBuf<float4> d_loss_grad;    // dL/d(image0) of s2d_loss_backward / s2d_step_loss
    // optimiser controls (s2d_set_optim / s2d_set_frozen, s2d_optim_rates.h): with either set the step launches the second
    // instantiation of the Adam kernel (adam_args)
    bool has_optim = false;
    s2d_optim_config optim{};
    bool has_frozen = false;
    DevBuf<uint8_t> d_frozen;      // n bytes, non-zero = frozen; allocated by the first mask
    SeedScratch seed;              // the importance map of s2d_importance / s2d_seed_splats / s2d_reseed (s2d_seed.h), on first use
    ViewScratch view;              // the records, lists and image of s2d_view_splats / s2d_render_view (s2d_view.h), on first use
    PixelWeights weights;          // the weight plane of the losses (include/splat2d_weights.h, s2d_loss_weighted.h), on first use
    BackdropState backdrop;        // what image0 is composited over (include/splat2d_backdrop.h, s2d_backdrop.h), on first use
    DevBuf<DeviceStatus> d_status;
    DevBuf<PairCounters> d_counters;
    // pinned host mirrors
    HostBuf<DeviceStatus> h_status;

    // host-side state of the reference's main()
    float beta1t = 1.0f, beta2t = 1.0f; // main.cpp:274-275
    int iterations = 0;                 // main.cpp:278
    float good_beta1t = 1.0f, good_beta2t = 1.0f; // the three above at the last point known to be finite
    int good_iterations = 0;
    char err[512] = {0};
    S2D_LOCAL ~s2d_ctx() = default; // (named only to keep it out of the library's exports, like the owners it runs)
};

S2D_LOCAL inline int fail(s2d_ctx* c, int code, const char* fmt, ...)
{
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof(c->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define S2D_HIP(c, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail((c), S2D_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Declared behind a temporary device buffer that work queued on `stream` uses: the stream is idle before the buffer
// is freed, on whichever way the function is left.
struct S2D_LOCAL IdleAtExit {
    hipStream_t stream;
    ~IdleAtExit() { (void)hipStreamSynchronize(stream); }
};

S2D_LOCAL inline int use_device(s2d_ctx* c)
{
    S2D_HIP(c, hipSetDevice(c->device));
    return S2D_OK;
}

// Device memory -> host memory behind everything queued on the context's stream.  Waits.
S2D_LOCAL inline int read_back(s2d_ctx* c, void* dst, const void* src, size_t bytes)
{
    S2D_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

// A coverage context (S2D_CFG_COVERAGE): image0.w, the target's .w and an image gradient's .w are the coverage channel.
S2D_LOCAL inline bool coverage(const s2d_ctx* c) { return (c->cfg.flags & S2D_CFG_COVERAGE) != 0; }
// What a coverage context has no kernels for (`who`: a call's name).  S2D_E_INVALID, before any device work.
S2D_LOCAL inline int coverage_refused(s2d_ctx* c, const char* who)
{
    if (coverage(c)) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_COVERAGE", who);
    return S2D_OK;
}

// What has no kernels over a backdrop (`who`: a call's name).  S2D_E_INVALID, before any device work.
S2D_LOCAL inline int backdrop_refused(s2d_ctx* c, const char* who)
{
    if (c->backdrop.set()) return fail(c, S2D_E_INVALID, "%s: not available while a backdrop is set (s2d_set_backdrop(ctx, NULL) removes it)", who);
    return S2D_OK;
}

// What cannot follow a pixel-weight plane (`who`: a call's name, `why`: what it would need).  S2D_E_INVALID, before any device work.
S2D_LOCAL inline int weights_refused(s2d_ctx* c, const char* who, const char* why)
{
    if (c->weights.set())
        return fail(c, S2D_E_INVALID, "%s: not available while pixel weights are set (%s; s2d_set_pixel_weights(ctx, NULL) removes them)", who, why);
    return S2D_OK;
}

S2D_LOCAL inline double mse_norm(const s2d_ctx* c) { return (double)((long long)c->g.H * c->g.W * 3); }

S2D_LOCAL inline size_t slab_pixels(const s2d_ctx* c) { return (size_t)c->g.W * (size_t)(c->g.row_end - c->g.row_begin); }

// `who` (a call's name) works on the whole image and on every splat, and has_reference_order == false: has no
// reference-order variant.  S2D_E_INVALID, before any device work.
S2D_LOCAL inline int whole_scene_refused(s2d_ctx* c, const char* who, bool has_reference_order)
{
    if (c->g.row_begin != 0 || c->g.row_end != c->g.H) return fail(c, S2D_E_INVALID, "%s: the whole image is needed, this context owns a row slab", who);
    if (c->state.kind() == SplatState::Subset::Slab) // (an alive set is no obstacle: a dead row does not exist for the passes)
        return fail(c, S2D_E_INVALID, "%s: every splat is needed, this context holds a subset (s2d_halo_commit)", who);
    if (!has_reference_order && c->surface.reference_order()) return fail(c, S2D_E_INVALID, "%s: not available with S2D_CFG_REFERENCE_ORDER", who);
    return S2D_OK;
}

// ---- what s2d_api_view.hip shares with s2d_api_coarse.hip (s2d_step_view runs a view's pass per iteration) -----------------
// A failed allocation of the view's scratch as the context's error (hipSuccess: S2D_OK).
S2D_LOCAL int view_alloc(s2d_ctx* c, hipError_t e, const char* what);
// What a pass with a backward walk through a view (`who`) refuses (S2D_E_INVALID): for the configuration, for the context.
S2D_LOCAL int view_pass_config_refused(s2d_ctx* c, const s2d_view_config* cfg, const char* who);
S2D_LOCAL int view_pass_context_refused(s2d_ctx* c, const char* who);
// The records, the projection and the lists of the view (queued, but for the one wait of a list build).
S2D_LOCAL int view_lists(s2d_ctx* c, const s2d_view_config* cfg);
// What every such pass starts with: the lists, the zeroed gradients of the view's records, the raster scratch, `walk` filled.
S2D_LOCAL int view_backward_prepare(s2d_ctx* c, const s2d_view_config* cfg, bool need_opacity_grad, RasterArgs* walk, float** grads);
// ... and ends with: those gradients through the adjoint of the record transform, added into the context's gradient buffer.
S2D_LOCAL int view_adjoint(s2d_ctx* c, const s2d_view_config* cfg, const float* record_grads);

// ---- what s2d_api_placement.hip shares with s2d_api_alive.hip (s2d_grow seeds the rows it brings to life) ---------------
// Everything the seeding calls (`who`) refuse for the configuration or the context, before any device work (S2D_E_INVALID),
// then what they refuse for the order of calls (S2D_E_STATE).
S2D_LOCAL int seed_refused(s2d_ctx* c, const s2d_seed_config* cfg, const char* who, bool has_reference_order = true);
S2D_LOCAL int seed_state_refused(s2d_ctx* c, const s2d_seed_config* cfg);
// The map of the current images (queued) and its total (waits).
S2D_LOCAL int seed_map(s2d_ctx* c, const s2d_seed_config* cfg, SeedMap* map, uint64_t* total);
// The rows ids_device[0 .. count) (distinct, in range; null: 0 .. count - 1) drawn from `map` (total > 0) and written (queued;
// rows_replaced).
S2D_LOCAL int seed_place(s2d_ctx* c, const s2d_seed_config* cfg, const SeedMap& map, uint64_t total, const int32_t* ids_device, int count);
// The host copy of the density statistics (n x 3) with the rows that are not alive set to NaN, which makes a row neither
// starved nor a donor for the planners of s2d_density.h.  Waits; nothing to do without an alive set.
S2D_LOCAL int mask_dead_stats(s2d_ctx* c, float* stats);
