// s2d_api.hip -- the C ABI of include/splat2d.h: the context's life, what goes in and comes out of it (target, splats,
// moments, image, gradients, traces, statistics), and the pass entry points, which check their arguments, select the
// device and call the sequence (s2d_sequence.h).  The loss passes, placement, slab ownership and the test hooks have units
// of their own (s2d_api_loss.hip, s2d_api_placement.hip, s2d_api_rows.hip, s2d_api_test.hip).
#include "s2d_ctx.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <new>

namespace {

// The image crosses the ABI as floats; a context with S2D_CFG_FP16_IMAGES keeps halves (round to nearest even) and
// converts on the way, through a temporary where the other side is host memory.
// The whole target (main.cpp:254-259) -> imageRef; a slab context uploads and keeps its own rows only.  Waits.
int upload_target(s2d_ctx* c, const float* rgba32f)
{
    const size_t px = slab_pixels(c), bytes = px * sizeof(float4);
    const float* src = rgba32f + (size_t)c->g.row_begin * c->g.W * 4;
    if (c->half_images) {
        DevBuf<float4> tmp;
        S2D_HIP(c, tmp.alloc(px));
        const IdleAtExit idle{c->stream}; // (before tmp goes)
        S2D_HIP(c, hipMemcpyAsync(tmp, src, bytes, hipMemcpyHostToDevice, c->stream));
        S2D_HIP(c, launch_convert_f32_to_f16(tmp, c->d_ref, px, c->stream));
    } else {
        S2D_HIP(c, hipMemcpyAsync(c->d_ref, src, bytes, hipMemcpyHostToDevice, c->stream));
    }
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

// image0 (the rows of the slab) -> dst.  to_host: waits; otherwise dst is device memory and the copy is only queued.
int download_image0(s2d_ctx* c, float* dst, bool to_host)
{
    const size_t px = slab_pixels(c), bytes = px * sizeof(float4);
    if (!c->half_images) {
        S2D_HIP(c, hipMemcpyAsync(dst, c->d_image0, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    } else if (!to_host) {
        S2D_HIP(c, launch_convert_f16_to_f32(c->d_image0, reinterpret_cast<float4*>(dst), px, c->stream));
    } else {
        DevBuf<float4> tmp;
        S2D_HIP(c, tmp.alloc(px));
        const IdleAtExit idle{c->stream}; // (before tmp goes)
        S2D_HIP(c, launch_convert_f16_to_f32(c->d_image0, tmp, px, c->stream));
        S2D_HIP(c, hipMemcpyAsync(dst, tmp, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (to_host) S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_abi_version(void) { return S2D_ABI_VERSION; }

int s2d_create(const s2d_config* cfg, s2d_ctx** out)
{
    if (!cfg || !out || cfg->struct_size != sizeof(s2d_config)) return S2D_E_INVALID;
    *out = nullptr;
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->n_splats < 0 || cfg->width > 65536 || cfg->height > 65536)
        return S2D_E_INVALID;
    int rb = cfg->row_begin, re = cfg->row_end;
    if (rb == 0 && re == 0) re = cfg->height;
    if (rb < 0 || re > cfg->height || rb >= re || (rb % kTile) != 0) return S2D_E_INVALID;
    if ((cfg->flags & (S2D_CFG_EXACT_EXP | S2D_CFG_REFERENCE_ORDER)) && (cfg->flags & (S2D_CFG_COUNT_PAIRS | S2D_CFG_FP16_IMAGES)))
        return S2D_E_INVALID;
    // the coverage channel: kernels of the plain lists of a whole image, without counting and with exp_approx (s2d_raster_coverage.hip)
    if ((cfg->flags & S2D_CFG_COVERAGE) && ((cfg->flags & (S2D_CFG_COUNT_PAIRS | S2D_CFG_EXACT_EXP | S2D_CFG_REFERENCE_ORDER)) ||
                                            rb != 0 || re != cfg->height))
        return S2D_E_INVALID;

    s2d_ctx* c = new (std::nothrow) s2d_ctx();
    if (!c) return S2D_E_NOMEM;
    *out = c; // handed out even on failure so that s2d_last_error works; caller destroys it
    c->cfg = *cfg;
    c->n = cfg->n_splats;
    c->device = cfg->device;
    c->lr = cfg->training_rate > 0.0f ? cfg->training_rate : 0.05f; // main.cpp:715

    const Geometry g = c->g = make_geometry(cfg->width, cfg->height, rb, re);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(c, S2D_E_HIP, "no HIP device available (%s): this library has no CPU fallback", hipGetErrorString(e));
    if (c->device < 0 || c->device >= ndev) return fail(c, S2D_E_INVALID, "device %d out of range (%d devices)", c->device, ndev);
    S2D_HIP(c, hipSetDevice(c->device));
    if (cfg->stream) {
        c->stream = (hipStream_t)cfg->stream;
    } else {
        S2D_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }

    const size_t n = std::max<size_t>((size_t)c->n, 1);           // >= 1 so that n == 0 still has buffers
    const size_t px = (size_t)g.W * (size_t)(g.row_end - g.row_begin); // pixels of the slab: all this context stores
    S2D_HIP(c, c->state.create(c->n, c->stream));
    S2D_HIP(c, c->d_grads_own.alloc(n * 9));
    c->d_grads = c->d_grads_own;
    S2D_HIP(c, c->d_scan_temp.alloc(scan_temp_words((int64_t)n)));
    const bool ref_order = (cfg->flags & S2D_CFG_REFERENCE_ORDER) != 0; // (alone decides the result: deterministic mode is off then)
    S2D_HIP(c, c->surface.create(g, n, (cfg->flags & S2D_CFG_GENERIC_BINNING) != 0,
                                 ref_order ? PairScratch::Mode::ReferenceOrder : (cfg->flags & S2D_CFG_DETERMINISTIC) ? PairScratch::Mode::Deterministic
                                           : PairScratch::Mode::Atomic, c->stream));
    c->ranges.create(g, c->stream);
    c->half_images = (cfg->flags & S2D_CFG_FP16_IMAGES) != 0;
    c->pixel_bytes = c->half_images ? 8 : sizeof(float4);
    S2D_HIP(c, c->d_image0.alloc(px * c->pixel_bytes));
    S2D_HIP(c, c->d_ref.alloc(px * c->pixel_bytes));
    S2D_HIP(c, c->d_status.alloc(1));
    S2D_HIP(c, c->trace.create(g.num_tiles, c->n, c->d_status, c->stream));
    c->density.create(c->n, c->stream);
    S2D_HIP(c, c->d_counters.alloc(1));
    S2D_HIP(c, c->reuse.create(cfg->rebin_interval, cfg->rebin_margin, c->stream));
    S2D_HIP(c, c->h_status.alloc(1, hipHostMallocDefault));

    S2D_HIP(c, hipMemsetAsync(c->d_grads_own, 0, n * 9 * sizeof(float), c->stream));
    S2D_HIP(c, hipMemsetAsync(c->d_image0, 0, px * c->pixel_bytes, c->stream));
    S2D_HIP(c, hipMemsetAsync(c->d_ref, 0, px * c->pixel_bytes, c->stream));
    S2D_HIP(c, hipMemsetAsync(c->d_counters, 0, sizeof(PairCounters), c->stream));
    *c->h_status = kFreshStatus;
    S2D_HIP(c, hipMemcpyAsync(c->d_status, c->h_status, sizeof(DeviceStatus), hipMemcpyHostToDevice, c->stream));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    // ~16 tiles per splat at init() scales; grown on demand
    int rc = ensure_pair_capacity(c, std::max<uint64_t>((uint64_t)n * 20, 1 << 16));
    if (rc != S2D_OK) return rc;
    return S2D_OK;
}

void s2d_destroy(s2d_ctx* c)
{
    if (!c) return;
    // the buffers, pinned mirrors and events go with their members: on the context's device, behind everything queued on
    // the stream, and before a stream of the context's own (also when the device cannot be selected: freeing needs none)
    if (hipSetDevice(c->device) == hipSuccess && c->stream) (void)hipStreamSynchronize(c->stream);
    const hipStream_t own = c->own_stream ? c->stream : nullptr;
    delete c;
    if (own) (void)hipStreamDestroy(own);
}

const char* s2d_last_error(const s2d_ctx* c) { return c ? c->err : "null context"; }

int s2d_set_target(s2d_ctx* c, const float* rgba32f)
{
    if (!c || !rgba32f) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (int rc = upload_target(c, rgba32f)) return rc;
    target_replaced(c);
    return S2D_OK;
}

int s2d_set_target_synthetic(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, launch_synthetic_target(c->d_ref, c->half_images, c->g.W, c->g.H, c->g.row_begin, c->g.row_end, c->stream));
    target_replaced(c);
    return S2D_OK;
}

int s2d_init_splats(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, c->trace.settle()); // (the iteration count is about to restart)
    if (c->state.kind() == SplatState::Subset::Alive) { // (a set of splats that no longer exist, like the frozen mask)
        S2D_HIP(c, c->state.clear_alive());
        alive_set_changed(c);
    }
    const SplatState::Arrays all = c->state.discard_all(); // every record is new
    S2D_HIP(c, launch_init_splats(all.splats, all.adams, c->n, c->g.W, c->g.H, c->stream));
    if (int rc = splats_replaced(c)) return rc;
    if (c->n > 0) S2D_HIP(c, hipMemsetAsync(c->d_grads, 0, (size_t)c->n * 9 * sizeof(float), c->stream));
    S2D_HIP(c, c->density.reset()); // (statistics of splats that no longer exist)
    c->has_frozen = false;          // (a mask of splats that no longer exist; the rates of s2d_set_optim stay)
    c->beta1t = c->good_beta1t = 1.0f; // main.cpp:283-284
    c->beta2t = c->good_beta2t = 1.0f;
    c->iterations = c->good_iterations = 0; // main.cpp:281
    return S2D_OK;
}

int s2d_set_splats(s2d_ctx* c, const s2d_splat* splats)
{
    if (!c || (!splats && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    SplatState::Arrays now; // (with the moments of the held splats: they must not be lost with the compact copy)
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, hipMemcpyAsync(now.splats, splats, (size_t)c->n * sizeof(s2d_splat), hipMemcpyHostToDevice, c->stream));
    if (int rc = splats_replaced(c)) return rc;
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

int s2d_get_splats(s2d_ctx* c, s2d_splat* splats)
{
    if (!c || (!splats && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    SplatState::Arrays now;
    S2D_HIP(c, c->state.current(&now));
    return read_back(c, splats, now.splats, (size_t)c->n * sizeof(s2d_splat));
}

int s2d_set_adam(s2d_ctx* c, const s2d_splat_adam* adams, float beta1t, float beta2t, int32_t iterations)
{
    if (!c || (!adams && c->n) || iterations < 0) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, c->trace.settle()); // (the iteration count is about to change)
    SplatState::Arrays now; // (with the parameters of the held splats: they must not be lost with the compact copy)
    S2D_HIP(c, c->state.current(&now));
    S2D_HIP(c, hipMemcpyAsync(now.adams, adams, (size_t)c->n * sizeof(s2d_splat_adam), hipMemcpyHostToDevice, c->stream));
    if (int rc = moments_replaced(c)) return rc;
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    c->beta1t = c->good_beta1t = beta1t;
    c->beta2t = c->good_beta2t = beta2t;
    c->iterations = c->good_iterations = iterations;
    return S2D_OK;
}

int s2d_get_adam(s2d_ctx* c, s2d_splat_adam* adams, float* beta1t, float* beta2t, int32_t* iterations)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (adams) {
        SplatState::Arrays now;
        S2D_HIP(c, c->state.current(&now));
        if (int rc = read_back(c, adams, now.adams, (size_t)c->n * sizeof(s2d_splat_adam))) return rc;
    }
    if (beta1t) *beta1t = c->beta1t;
    if (beta2t) *beta2t = c->beta2t;
    if (iterations) *iterations = c->iterations;
    return S2D_OK;
}

int s2d_forward(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    return queue_forward(c);
}

int s2d_get_image_rows(s2d_ctx* c, float* rgba32f_rows)
{
    if (!c || !rgba32f_rows) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    return download_image0(c, rgba32f_rows, true);
}

int s2d_get_image(s2d_ctx* c, float* rgba32f)
{
    if (!c || !rgba32f) return S2D_E_INVALID;
    // a full-size image goes back (main.cpp:794 uploads all of image0): this context's rows, zeros elsewhere
    const size_t row_floats = (size_t)c->g.W * 4;
    std::memset(rgba32f, 0, (size_t)c->g.row_begin * row_floats * sizeof(float));
    std::memset(rgba32f + (size_t)c->g.row_end * row_floats, 0, (size_t)(c->g.H - c->g.row_end) * row_floats * sizeof(float));
    return s2d_get_image_rows(c, rgba32f + (size_t)c->g.row_begin * row_floats);
}

int s2d_forward_backward(s2d_ctx* c, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    if (flags & S2D_BWD_DENSITY_STATS)
        return fail(c, S2D_E_INVALID, "the fused launch has no density-statistics variant: s2d_forward, then s2d_backward with the flag");
    if (int rc = use_device(c)) return rc;
    return queue_forward_backward(c, !(flags & S2D_BWD_SKIP_OPACITY_GRAD), !(flags & S2D_FB_SKIP_IMAGE));
}

int s2d_backward(s2d_ctx* c, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    WalkFlags wf;
    if (int rc = parse_walk_flags(c, flags, false, &wf)) return rc;
    if (int rc = use_device(c)) return rc;
    return queue_backward(c, wf.need_opacity_grad, nullptr, wf.density);
}

int s2d_backward_image_grads(s2d_ctx* c, const float* dimage_rows_device, uint32_t flags)
{
    if (!c || !dimage_rows_device) return S2D_E_INVALID;
    if ((uintptr_t)dimage_rows_device & 15u) return fail(c, S2D_E_INVALID, "the image gradient must be 16-byte aligned");
    if (c->cfg.flags & S2D_CFG_COUNT_PAIRS)
        return fail(c, S2D_E_INVALID, "pair counting (S2D_CFG_COUNT_PAIRS) has no backward pass from a caller's image gradient");
    WalkFlags wf;
    if (int rc = parse_walk_flags(c, flags, false, &wf)) return rc;
    if (int rc = use_device(c)) return rc;
    return queue_backward(c, wf.need_opacity_grad, reinterpret_cast<const float4*>(dimage_rows_device), wf.density);
}

int s2d_set_splats_device(s2d_ctx* c, const float* splats_device)
{
    if (!c || (!splats_device && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    SplatState::Arrays now; // (with the moments of the held splats: they must not be lost with the compact copy)
    S2D_HIP(c, c->state.current(&now));
    if (c->n > 0)
        S2D_HIP(c, hipMemcpyAsync(now.splats, splats_device, (size_t)c->n * sizeof(s2d_splat), hipMemcpyDeviceToDevice, c->stream));
    return splats_replaced_from_device(c);
}

int s2d_get_image_rows_device(s2d_ctx* c, float* rgba32f_rows_device)
{
    if (!c || !rgba32f_rows_device) return S2D_E_INVALID;
    if ((uintptr_t)rgba32f_rows_device & 15u) return fail(c, S2D_E_INVALID, "the image buffer must be 16-byte aligned");
    if (int rc = use_device(c)) return rc;
    return download_image0(c, rgba32f_rows_device, false);
}

int s2d_get_grads(s2d_ctx* c, s2d_splat* dsplats)
{
    if (!c || (!dsplats && c->n)) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    return read_back(c, dsplats, c->d_grads, (size_t)c->n * sizeof(s2d_splat));
}

int s2d_adam_step(s2d_ctx* c, uint32_t flags)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (int rc = queue_adam(c, flags)) return rc;
    return S2D_OK;
}

int s2d_step(s2d_ctx* c, int32_t iters, uint32_t flags, double* mse_out)
{
    if (!c || iters < 0) return S2D_E_INVALID;
    return run_steps(c, iters, flags, nullptr, nullptr, mse_out);
}

int s2d_get_mse(s2d_ctx* c, double* mse)
{
    if (!c || !mse) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (c->trace.last_iteration() < 0) return fail(c, S2D_E_STATE, "no backward pass has run yet");
    double v = 0.0;
    S2D_HIP(c, c->trace.read(c->trace.last_iteration(), 1, &v));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    *mse = v / mse_norm(c);
    return S2D_OK;
}

int s2d_bind_grads_device(s2d_ctx* c, void* grads_device)
{
    if (!c) return S2D_E_INVALID;
    if ((uintptr_t)grads_device & 15u) return fail(c, S2D_E_INVALID, "the gradient buffer must be 16-byte aligned");
    c->d_grads = grads_device ? (float*)grads_device : c->d_grads_own;
    return S2D_OK;
}

void* s2d_grads_device_ptr(s2d_ctx* c) { return c ? (void*)c->d_grads : nullptr; }

void* s2d_stream(s2d_ctx* c) { return c ? (void*)c->stream : nullptr; }

int s2d_get_sqerr_trace(s2d_ctx* c, int32_t first_iteration, int32_t count, double* out)
{
    if (!c || !out || count < 0 || first_iteration < 0 || count > SqerrTrace::kCapacity) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    S2D_HIP(c, c->trace.read(first_iteration, count, out));
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

int s2d_synchronize(s2d_ctx* c)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    return check_status(c);
}

int s2d_get_stats(s2d_ctx* c, s2d_stats* out)
{
    // the struct as its first version (ABI 2) ends with bwd_quadrant_execs: a caller must have at least that
    if (!c || !out || out->struct_size < (uint32_t)(offsetof(s2d_stats, bwd_quadrant_execs) + sizeof(uint64_t))) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    PairCounters pc;
    S2D_HIP(c, hipMemcpyAsync(&pc, c->d_counters, sizeof(pc), hipMemcpyDeviceToHost, c->stream));
    if (int rc = queue_status_read(c)) return rc;
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    // filled in a full-size copy, handed back at the caller's size: a caller built against an older, shorter struct is
    // never written past its end
    const uint32_t caller_size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(s2d_stats));
    s2d_stats full;
    s2d_stats* const dst = out;
    out = &full;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = caller_size;
    out->pairs_binned = c->surface.lists().pairs();
    out->pairs_capacity = c->surface.lists().capacity();
    out->rebins = c->surface.lists().builds();
    out->fwd_visited = pc.fwd_visited; out->fwd_active = pc.fwd_active;
    out->bwd_visited = pc.bwd_visited; out->bwd_active = pc.bwd_active;
    out->fwd_staged = pc.fwd_staged; out->bwd_staged = pc.bwd_staged;
    out->fwd_wave_execs = pc.fwd_wave_execs; out->bwd_wave_execs = pc.bwd_wave_execs;
    for (int k = 0; k < 65; k++) out->bwd_lane_hist[k] = pc.bwd_lane_hist[k];
    out->fwd_staged_hit = pc.fwd_staged_hit;
    out->fwd_rows_hit = pc.fwd_rows_hit;
    out->bwd_quadrant_execs = pc.bwd_quadrant_execs;
    out->iterations = c->iterations;
    out->first_nonfinite_iteration = c->h_status->nonfinite ? c->h_status->first_nonfinite_iter : -1;
    std::memcpy(dst, &full, caller_size);
    return S2D_OK;
}

int s2d_get_rebuild_count(const s2d_ctx* c, uint64_t* rebuilds)
{
    if (!c || !rebuilds) return S2D_E_INVALID;
    *rebuilds = c->surface.lists().builds();
    return S2D_OK;
}

int s2d_debug_get_tile_lists(s2d_ctx* c, int32_t* tiles_x, int32_t* tiles_y, uint32_t* offsets,
                             int64_t offsets_capacity, uint32_t* list, int64_t list_capacity)
{
    if (!c) return S2D_E_INVALID;
    if (int rc = use_device(c)) return rc;
    if (!c->fresh.lists()) return fail(c, S2D_E_STATE, "tile lists not built yet (run s2d_forward)");
    if (tiles_x) *tiles_x = c->g.tiles_x;
    if (tiles_y) *tiles_y = c->g.tiles_y;
    if (offsets) {
        if (offsets_capacity < c->g.num_tiles + 1) return S2D_E_INVALID;
        S2D_HIP(c, hipMemcpyAsync(offsets, c->surface.lists().tile_off(), (size_t)(c->g.num_tiles + 1) * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, c->stream));
    }
    if (list) {
        if (list_capacity < (int64_t)c->surface.lists().pairs()) return S2D_E_INVALID;
        S2D_HIP(c, hipMemcpyAsync(list, c->surface.lists().list(), (size_t)c->surface.lists().pairs() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    S2D_HIP(c, hipStreamSynchronize(c->stream));
    return S2D_OK;
}

} // extern "C"
