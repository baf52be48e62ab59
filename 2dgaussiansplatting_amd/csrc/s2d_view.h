// s2d_view.h -- view rendering on the device (include/splat2d.h, s2d_view_splats / s2d_render_view):
// launch declarations of s2d_view.hip and the owner of everything a view allocates.
//
// A view is drawn in four steps on the context's stream: the transform kernel fills an n x 9 buffer with the records as the
// view rasterises them (s2d_view_math.h); project_kernel (mode 0, margin 0) turns them into ProjRec and exact rectangles in the
// view's Geometry; a TileLists instance of the view's own builds the lists; the view raster kernel walks them and writes the
// caller's buffer.  Nothing of the context's training state is written.
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
};
// The forward walk of every tile of the grid, resolved to output pixels inside the workgroup: writes nothing but `out`.
hipError_t launch_view_raster(const ViewRasterArgs& a, hipStream_t stream);

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
    void release(hipStream_t stream)
    {
        (void)hipStreamSynchronize(stream);
        lists_.reset();
        splats_.release(), proj_.release(), rects_.release(), counts_.release(), offsets_.release(), image_.release();
        g_ = Geometry{};
    }
    bool has_lists(const Geometry& g) const { return lists_ && g.W == g_.W && g.H == g_.H && lists_->list() != nullptr; }
    bool allocated() const { return lists_ || splats_ || image_; }

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
    std::unique_ptr<TileLists> lists_;
    Geometry g_{};
};

} // namespace s2d
