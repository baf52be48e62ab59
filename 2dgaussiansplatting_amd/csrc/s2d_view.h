// s2d_view.h -- view rendering on the device (include/splat2d.h, s2d_view_splats / s2d_render_view):
// launch declarations of s2d_view.hip and the owner of everything a view allocates.
//
// A view is drawn in four steps on the context's stream: the transform kernel fills an n x 9 buffer with the records as the
// view rasterises them (s2d_view_math.h); project_kernel (mode 0, margin 0) turns them into ProjRec and exact rectangles in the
// view's Geometry; the views' own RasterSurface (s2d_context.h) builds the lists; the view raster kernel walks them and writes the
// caller's buffer.  Nothing of the context's training state is written.
//
// The backward pass through a view (s2d_view_backward_device; s2d_view_gradient.hip) takes the same first
// three steps, then view_gradient_kernel walks the lists forward and backward and leaves the gradients of the view's records in
// an n x 9 buffer of the view's own, and view_adjoint_kernel adds them, taken back through the transform, into the context's
// gradient buffer -- the one thing of the context's that a view ever writes.
#pragma once

#include "s2d_context.h"
#include "s2d_device.h"
#include "s2d_owned.h"
#include "s2d_view_math.h"

#include <type_traits>

namespace s2d {

// The raster grid of a view: (out_width * samples) x (out_height * samples), whole, not a slab.
inline Geometry view_geometry(int out_width, int out_height, int samples)
{
    return make_geometry(out_width * samples, out_height * samples, 0, out_height * samples);
}

// out[i] = view_row(x, splats[i]) for the n rows of the capacity, dead ones included.
hipError_t launch_view_transform(const float* splats, int n, ViewXform x, float* out, hipStream_t stream);

struct ViewRasterArgs {
    RasterArgs walk;        // of it: tile_off, list, proj, g (the raster grid: out * samples), exact_exp, coverage (never with exact_exp)
    void* out = nullptr;    // out_height * out_width pixels: RGBA32F (16-byte aligned) or, with rgba8, 4 bytes each
    int out_width = 0;
    int samples = 1;        // 1, 2 or 4 per axis
    bool rgba8 = false;
    float rgb[3] = {0.0f, 0.0f, 0.0f}; // launch_backdrop_view: the constant backdrop
};
// The sample walk of every tile of the grid, resolved to output pixels inside the workgroup: writes nothing but `out`.
hipError_t launch_view_raster(const ViewRasterArgs& a, hipStream_t stream);
// The same with c += T * rgb per sample before the resolve (s2d_backdrop.hip; exp_approx, no coverage).
hipError_t launch_backdrop_view(const ViewRasterArgs& a, hipStream_t stream);

// samples per axis -> a compile-time constant: f(std::integral_constant<int, S>{}) for S = 1, 2, 4 and what it returns; every
// launch of a view kernel goes through here, so which S exist is decided here and nowhere else.
template <typename F>
inline hipError_t with_samples(int samples, F&& f)
{
    switch (samples) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return hipErrorInvalidValue; // a missing kernel is an error
    }
}

#if defined(__HIPCC__)
// One level of the resolve: the 2 x 2 block whose top-left lane is this one, DX / DY = the lane distance of its right / lower
// neighbour.  Every lane runs it; the value is the block's only in its top-left lane.
template <int DX, int DY>
__device__ __forceinline__ float resolve_level(float v)
{
    const float h = v + __shfl_xor(v, DX, 64);  // p00 + p01 (p10 + p11 in the lane below)
    return (h + __shfl_xor(h, DY, 64)) * 0.25f; // view_resolve4
}
#endif

struct ViewGradientArgs {
    // of it: tile_off, list, proj, the hand-over, grads (n x 9: the gradients of the view's records, ACCUMULATED), g (the raster
    // grid: out * samples), det (det.now != 0: partial gradients into the slots, then the gather kernel), exact_exp, need_opacity_grad
    RasterArgs walk;
    const float4* src = nullptr;    // out_height * out_width RGBA32F, .w ignored: dL/d(view), or with from_target the target
    int out_width = 0;
    int samples = 1;                // 1, 2 or 4 per axis
    bool from_target = false;
};
// Forward walk, adjoint of the resolve and backward walk of every tile of the grid (and deterministic mode's gather).
hipError_t launch_view_gradient(const ViewGradientArgs& a, hipStream_t stream);
// grads[i] += view_row_adjoint(x, splats[i], view_grads[i]) for the n rows of the capacity; rows with held[i] == 0 are skipped
// (held == nullptr: none is).
hipError_t launch_view_adjoint(const float* splats, const uint8_t* held, int n, ViewXform x, const float* view_grads, float* grads,
                               hipStream_t stream);

// Coarse-to-fine fitting (include/splat2d_coarse.h; s2d_view_fit.hip): view_gradient_kernel's pass from a
// target (a.from_target, a.src the target) with the view's squared error per tile into a.walk.tile_sqerr (one double per tile of
// g: every tile's is stored), and deterministic mode's gather.
hipError_t launch_view_fit(const ViewGradientArgs& a, hipStream_t stream);
// out[j][i] = view_target_pixel (s2d_view_target_math.h) of the W x H image at ref (half_images: 4 x fp16 per pixel, else RGBA32F).
hipError_t launch_view_target(const void* ref, bool half_images, int W, int H, float origin_x, float origin_y, float zoom, int out_width,
                              int out_height, float4* out, hipStream_t stream);

// The window of a view's own target: what s2d_view_target_device depends on besides the context's target.
struct ViewWindow {
    int out_width = 0, out_height = 0;
    float origin_x = 0.0f, origin_y = 0.0f, zoom = 0.0f;
    bool operator==(const ViewWindow& o) const
    {
        return out_width == o.out_width && out_height == o.out_height && origin_x == o.origin_x && origin_y == o.origin_y && zoom == o.zoom;
    }
};

// What views allocate, on first use, and keep between calls (a context that never renders a view pays nothing): the n x 9 records and
// their gradients, the device image behind s2d_render_view, one RasterSurface for the raster grid of the latest call, and for
// s2d_step_view the tile errors, the ring of their sums and the library's own target of the latest window.
class S2D_LOCAL ViewScratch {
public:
    static constexpr int kFitRing = 256; // iterations of s2d_step_view queued between two reads of their squared errors

    // The tile errors of a view_fit pass over `num_tiles` tiles, with the zeroed scratch sqerr_reduce expects behind them (the
    // reduction leaves it zero), and the ring of per-iteration sums.
    hipError_t fit_errors(int num_tiles, hipStream_t stream, SqerrJob* job, double** tile_sqerr)
    {
        const size_t want = (size_t)num_tiles + kSqerrScratchDoubles;
        if (fit_tiles_ != num_tiles || !tile_sqerr_) {
            if (tile_sqerr_) (void)hipStreamSynchronize(stream);
            fit_tiles_ = 0;
            S2D_TRY(tile_sqerr_.alloc(want));
            S2D_TRY(hipMemsetAsync(tile_sqerr_, 0, want * sizeof(double), stream));
            fit_tiles_ = num_tiles;
        }
        if (!fit_ring_) S2D_TRY(fit_ring_.alloc(kFitRing));
        *tile_sqerr = tile_sqerr_;
        *job = SqerrJob{tile_sqerr_, num_tiles, fit_ring_, tile_sqerr_ + num_tiles}; // (out: the ring's first slot; the caller picks its own)
        return hipSuccess;
    }
    // The library's own target of window `w` (out_height x out_width RGBA32F); *current: it holds that window of the context's
    // target as it stands, otherwise the caller fills it (queued) and says own_target_built().
    hipError_t own_target(const ViewWindow& w, hipStream_t stream, float4** out, bool* current)
    {
        const size_t pixels = (size_t)w.out_width * (size_t)w.out_height;
        if (pixels > target_.capacity()) {
            if (target_) (void)hipStreamSynchronize(stream);
            target_current_ = false;
            S2D_TRY(target_.alloc(pixels));
        }
        *current = target_current_ && window_ == w;
        if (!*current) target_current_ = false, window_ = w;
        *out = target_;
        return hipSuccess;
    }
    void own_target_built() { target_current_ = true; }
    void target_stale() { target_current_ = false; } // the context's target was replaced (target_replaced, s2d_sequence.hip)

    // The n x 9 records of the view.
    hipError_t rows(size_t n, float** out)
    {
        if (!splats_) S2D_TRY(splats_.alloc(n * 9));
        *out = splats_;
        return hipSuccess;
    }
    // The device image behind s2d_render_view's host buffer.
    hipError_t image(size_t bytes, void** out)
    {
        S2D_TRY(image_.reserve((bytes + 15) / 16));
        *out = (uint4*)image_;
        return hipSuccess;
    }
    // The n x 9 gradients of the view's records, zeroed (queued).
    hipError_t grads(size_t n, hipStream_t stream, float** out)
    {
        if (!grads_) S2D_TRY(grads_.alloc(n * 9));
        *out = grads_;
        return hipMemsetAsync(grads_, 0, std::max<size_t>(n, 1) * 9 * sizeof(float), stream);
    }
    void release(hipStream_t stream)
    {
        (void)hipStreamSynchronize(stream);
        surface_ = RasterSurface();
        splats_.release(), image_.release(), grads_.release();
        tile_sqerr_.release(), fit_ring_.release(), target_.release();
        fit_tiles_ = 0, target_current_ = false;
    }
    bool has_lists(const Geometry& g) const { return surface_.on(g) && surface_.lists().list() != nullptr; }
    bool allocated() const { return surface_.allocated() || splats_ || image_ || grads_ || tile_sqerr_ || fit_ring_ || target_; }
    RasterSurface& surface() { return surface_; } // of the latest call's grid; whoever calls on another creates it again

private:
    DevBuf<float> splats_;
    DevBuf<uint4> image_;
    DevBuf<float> grads_; // [n][9]: gradients of the view's records
    RasterSurface surface_;
    DevBuf<double> tile_sqerr_; // [fit_tiles_ + kSqerrScratchDoubles]
    DevBuf<double> fit_ring_;   // [kFitRing]
    int fit_tiles_ = 0;
    DevBuf<float4> target_;     // the library's own target of window_
    ViewWindow window_;
    bool target_current_ = false;
};

} // namespace s2d
