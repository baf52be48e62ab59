// s2d_view.h -- view rendering on the device (include/splat2d.h, s2d_view_splats / s2d_render_view):
// launch declarations of s2d_view.hip and the owner of everything a view allocates.
//
// A view is drawn in four steps on the context's stream: the transform kernel fills an n x 9 buffer with the records as the
// view rasterises them (s2d_view_math.h); project_kernel (mode 0, margin 0) turns them into ProjRec and exact rectangles in the
// view's Geometry; a TileLists instance of the view's own builds the lists; the view raster kernel walks them and writes the
// caller's buffer.  Nothing of the context's training state is written.
//
// The backward pass through a view (s2d_view_backward_device; s2d_view_gradient.hip) takes the same first
// three steps, then view_gradient_kernel walks the lists forward and backward and leaves the gradients of the view's records in
// an n x 9 buffer of the view's own, and view_adjoint_kernel adds them, taken back through the transform, into the context's
// gradient buffer -- the one thing of the context's that a view ever writes.
#pragma once

#include <memory>

#include "s2d_device.h"
#include "s2d_lists.h"
#include "s2d_owned.h"
#include "s2d_view_math.h"

namespace s2d {

// The raster grid of a view: (out_width * samples) x (out_height * samples), whole, not a slab.
inline Geometry view_geometry(int out_width, int out_height, int samples)
{
    Geometry g{};
    g.W = out_width * samples;
    g.H = out_height * samples;
    g.row_begin = 0;
    g.row_end = g.H;
    g.tiles_x = (g.W + kTile - 1) / kTile;
    g.trow0 = 0;
    g.tiles_y = (g.H + kTile - 1) / kTile;
    g.num_tiles = g.tiles_x * g.tiles_y;
    return g;
}

// out[i] = view_row(x, splats[i]) for the n rows of the capacity, dead ones included.
hipError_t launch_view_transform(const float* splats, int n, ViewXform x, float* out, hipStream_t stream);

struct ViewRasterArgs {
    const uint32_t* tile_off = nullptr;
    const uint32_t* list = nullptr;
    const ProjRec* proj = nullptr;
    void* out = nullptr;    // out_height * out_width pixels: RGBA32F (16-byte aligned) or, with rgba8, 4 bytes each
    Geometry g{};           // the raster grid: out * samples
    int out_width = 0;
    int samples = 1;        // 1, 2 or 4 per axis
    bool rgba8 = false;
    bool exact_exp = false;
    bool coverage = false;  // .w (the alpha byte) is the coverage channel, S2D_CFG_COVERAGE; never with exact_exp
};
// The forward walk of every tile of the grid, resolved to output pixels inside the workgroup: writes nothing but `out`.
hipError_t launch_view_raster(const ViewRasterArgs& a, hipStream_t stream);

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
    const uint32_t* tile_off = nullptr;
    const uint32_t* list = nullptr;
    const ProjRec* proj = nullptr;
    const float4* src = nullptr;    // out_height * out_width RGBA32F, .w ignored: dL/d(view), or with from_target the target
    // the forward -> backward hand-over of the view (ViewScratch), as RasterArgs describes the context's
    unsigned long long* wave_masks = nullptr;
    uint32_t* exec_list = nullptr;
    uint32_t* tile_exec = nullptr;
    uint32_t* retire_hint = nullptr;
    float* grads = nullptr;         // n x 9: the gradients of the view's records, ACCUMULATED
    Geometry g{};                   // the raster grid: out * samples
    int out_width = 0;
    int samples = 1;                // 1, 2 or 4 per axis
    DetGather det{};                // det.now != 0: partial gradients into the view's slots, then the gather kernel
    bool exact_exp = false;
    bool need_opacity_grad = true;
    bool from_target = false;
};
// Forward walk, adjoint of the resolve and backward walk of every tile of the grid (and deterministic mode's gather).
hipError_t launch_view_gradient(const ViewGradientArgs& a, hipStream_t stream);
// grads[i] += view_row_adjoint(x, splats[i], view_grads[i]) for the n rows of the capacity; rows with held[i] == 0 are skipped
// (held == nullptr: none is).
hipError_t launch_view_adjoint(const float* splats, const uint8_t* held, int n, ViewXform x, const float* view_grads, float* grads,
                               hipStream_t stream);

// What views allocate, on first use, and keep between calls (a context that never renders a view pays nothing).  The lists
// belong to one raster grid: another grid replaces them.  Whoever replaces or releases makes the stream idle first.
class S2D_LOCAL ViewScratch {
public:
    // The n x 9 records of the view.
    hipError_t rows(size_t n, float** out)
    {
        if (!splats_) S2D_TRY(splats_.alloc(n * 9));
        *out = splats_;
        return hipSuccess;
    }
    // The per-splat arrays and the list builder for grid `g`.
    hipError_t lists_for(const Geometry& g, size_t n, bool generic, hipStream_t stream)
    {
        if (lists_ && g.W == g_.W && g.H == g_.H) return hipSuccess;
        if (lists_) {
            S2D_TRY(hipStreamSynchronize(stream));
            lists_.reset();
            tile_exec_.release(), retire_hint_.release(); // (per tile of the grid that goes)
        }
        if (!proj_) {
            S2D_TRY(proj_.alloc(n));
            S2D_TRY(rects_.alloc(n));
            S2D_TRY(counts_.alloc(n));
            S2D_TRY(offsets_.alloc(n));
        }
        std::unique_ptr<TileLists> fresh(new TileLists());
        S2D_TRY(fresh->create(g, n, generic));
        lists_ = std::move(fresh);
        g_ = g;
        return hipSuccess;
    }
    // Room for `pairs` (tile, splat) pairs in the lists' buffers (which exist from the first call on, also for no pair).
    hipError_t pairs_for(uint64_t pairs, hipStream_t stream)
    {
        if (lists_->capacity() > 0 && pairs <= lists_->capacity()) return hipSuccess;
        uint64_t cap = std::max<uint64_t>(pairs + pairs / 4 + 4096, 1 << 16);
        if (cap > 0xFFFF0000ull) cap = 0xFFFF0000ull;
        S2D_TRY(hipStreamSynchronize(stream));
        lists_->release_pairs();
        return lists_->alloc_pairs(cap);
    }
    // The device image behind s2d_render_view's host buffer.
    hipError_t image(size_t bytes, void** out)
    {
        S2D_TRY(image_.reserve((bytes + 15) / 16));
        *out = (uint4*)image_;
        return hipSuccess;
    }
    // What a gradient pass over the current lists works on beside them (call behind pairs_for()): the n x 9 gradients of the
    // view's records, zeroed (queued); the forward -> backward hand-over, 36 bytes per pair of the lists' capacity, and the
    // per-tile words, the retirement hints unknown for a new grid; deterministic: the slots (kDetStride floats and a stamp per
    // pair of capacity), the per-splat `touched` words and a fresh epoch for this pass -- everything PairScratch keeps for the
    // context, for the view's rectangles and offsets.
    hipError_t gradient_for(size_t n, bool deterministic, hipStream_t stream, ViewGradientArgs* a)
    {
        if (!grads_) S2D_TRY(grads_.alloc(n * 9));
        S2D_TRY(hipMemsetAsync(grads_, 0, std::max<size_t>(n, 1) * 9 * sizeof(float), stream));
        if (!tile_exec_) {
            S2D_TRY(tile_exec_.alloc((size_t)g_.num_tiles));
            S2D_TRY(retire_hint_.alloc((size_t)g_.num_tiles));
            S2D_TRY(hipMemsetAsync(retire_hint_, 0xFF, (size_t)g_.num_tiles * sizeof(uint32_t), stream));
        }
        const uint64_t cap = lists_->capacity();
        if (handover_pairs_ != cap || (deterministic && !det_data_)) {
            S2D_TRY(hipStreamSynchronize(stream));
            handover_pairs_ = 0;
            S2D_TRY(wave_masks_.alloc((size_t)cap * 4));
            S2D_TRY(exec_list_.alloc((size_t)cap));
            if (deterministic) {
                S2D_TRY(det_data_.alloc((size_t)cap * kDetStride));
                S2D_TRY(stamp_.alloc((size_t)cap));
                S2D_TRY(hipMemsetAsync(stamp_, 0, (size_t)cap * sizeof(uint32_t), stream));
            }
            handover_pairs_ = cap;
        }
        if (deterministic && !det_touched_) {
            S2D_TRY(det_touched_.alloc(n));
            S2D_TRY(hipMemsetAsync(det_touched_, 0, std::max<size_t>(n, 1) * sizeof(uint32_t), stream));
        }
        a->wave_masks = wave_masks_, a->exec_list = exec_list_, a->tile_exec = tile_exec_, a->retire_hint = retire_hint_;
        a->grads = grads_;
        if (deterministic) a->det = DetGather{rects_, offsets_, counts_, det_data_, stamp_, det_touched_, ++epoch_, (int)n};
        return hipSuccess;
    }
    void release(hipStream_t stream)
    {
        (void)hipStreamSynchronize(stream);
        lists_.reset();
        splats_.release(), proj_.release(), rects_.release(), counts_.release(), offsets_.release(), image_.release();
        grads_.release(), wave_masks_.release(), exec_list_.release(), tile_exec_.release(), retire_hint_.release();
        det_data_.release(), stamp_.release(), det_touched_.release();
        handover_pairs_ = 0;
        g_ = Geometry{};
    }
    bool has_lists(const Geometry& g) const { return lists_ && g.W == g_.W && g.H == g_.H && lists_->list() != nullptr; }
    bool allocated() const { return lists_ || splats_ || image_ || grads_; }

    TileLists& lists() { return *lists_; }
    ProjRec* proj() const { return proj_; }
    TileRect* rects() const { return rects_; }
    uint32_t* counts() const { return counts_; }
    uint32_t* offsets() const { return offsets_; }

private:
    DevBuf<float> splats_;
    DevBuf<ProjRec> proj_;
    DevBuf<TileRect> rects_;
    DevBuf<uint32_t> counts_, offsets_;
    DevBuf<uint4> image_;
    // the gradient pass (gradient_for)
    DevBuf<float> grads_;                   // [n][9]: gradients of the view's records
    DevBuf<unsigned long long> wave_masks_; // [pair capacity][4]
    DevBuf<uint32_t> exec_list_;            // [pair capacity]
    DevBuf<uint32_t> tile_exec_, retire_hint_; // [tiles of the grid]
    DevBuf<float> det_data_;                // deterministic: [pair capacity][kDetStride]
    DevBuf<uint32_t> stamp_;                // deterministic: [pair capacity]
    DevBuf<uint32_t> det_touched_;          // deterministic: [n], zero between passes
    uint64_t handover_pairs_ = 0;           // pair capacity the hand-over (and the slots) were allocated for
    uint32_t epoch_ = 0;                    // stamps handed out so far (0 = never)
    std::unique_ptr<TileLists> lists_;
    Geometry g_{};
};

} // namespace s2d
