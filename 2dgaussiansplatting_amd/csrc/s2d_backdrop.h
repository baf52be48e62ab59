// s2d_backdrop.h -- a backdrop behind the splats (include/splat2d_backdrop.h): launch declarations of
// s2d_backdrop.hip and the owner of what a backdrop allocates.
//
// image0.c = C.c + (T_final * B.c): the forward walk of a backdrop context is backdrop_forward_kernel, which has T_final in a
// register at the store and also leaves it in a plane of its own; every other kernel of an iteration is the plain context's and
// works on image0 as stored.
#pragma once

#include "s2d_device.h"
#include "s2d_owned.h"

namespace s2d {

// What RasterArgs::backdrop points at (RasterPass::Forward of a context with a backdrop).
struct BackdropArgs {
    float rgb[3] = {0.0f, 0.0f, 0.0f}; // the constant
    const float4* plane = nullptr;     // != nullptr: W x H RGBA32F instead of the constant, .w ignored
    float* throughput = nullptr;       // W x H floats: T_final of every pixel
};
// uses of `a`: as raster_forward_kernel's (lists, hand-over, image0, g, status, abort_stamp, iteration, half_images) and a.backdrop
hipError_t launch_raster_backdrop(const RasterArgs& a, hipStream_t stream);

// (the view over a constant backdrop, launch_backdrop_view, takes a ViewRasterArgs and is declared with it: s2d_view.h)

constexpr int kBackdropGradBlocks = 256; // partial sums of s2d_backdrop_grads: at most this many workgroups, each a fixed set of pixels

struct BackdropGradArgs {
    const float* throughput = nullptr; // [pixels]
    const void* image0 = nullptr;      // upstream == nullptr: g = image0 - image_ref (half_images: 4 x fp16 per pixel)
    const void* image_ref = nullptr;
    const float4* upstream = nullptr;  // != nullptr: g
    bool half_images = false;
    size_t pixels = 0;
    float4* dplane = nullptr;          // may be nullptr: (T g_r, T g_g, T g_b, 0) per pixel
    double* partials = nullptr;        // may be nullptr (no sums wanted): [kBackdropGradBlocks][3] scratch
    double* sums = nullptr;            // with partials: [3]
};
hipError_t launch_backdrop_grads(const BackdropGradArgs& a, hipStream_t stream);

// The backdrop of a context: kind and colour on the host; the context's copy of a plane, the throughput plane and the scratch of
// the sums on the device, allocated by the first call that needs them and kept until the context goes.
class S2D_LOCAL BackdropState {
public:
    enum Kind { None = 0, Constant = 1, Plane = 2 };

    Kind kind() const { return kind_; }
    bool set() const { return kind_ != None; }
    const float* rgb() const { return args_.rgb; }
    // What a forward launch takes (nullptr: no backdrop).
    const BackdropArgs* args() const { return set() ? &args_ : nullptr; }
    const float* throughput() const { return throughput_; }

    void clear()
    {
        kind_ = None;
        args_ = BackdropArgs{};
    }
    hipError_t set_constant(const float* rgb, size_t pixels)
    {
        S2D_TRY(reserve_throughput(pixels));
        kind_ = Constant;
        for (int k = 0; k < 3; k++) args_.rgb[k] = rgb[k];
        args_.plane = nullptr;
        args_.throughput = throughput_;
        return hipSuccess;
    }
    // The plane is copied on `stream` (queued behind every pass that still reads the copy before it).
    hipError_t set_plane(const float* rgba32f_device, size_t pixels, hipStream_t stream)
    {
        S2D_TRY(reserve_throughput(pixels));
        if (!plane_) S2D_TRY(plane_.alloc(pixels));
        S2D_TRY(hipMemcpyAsync(plane_, rgba32f_device, pixels * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        kind_ = Plane;
        args_ = BackdropArgs{};
        args_.plane = plane_;
        args_.throughput = throughput_;
        return hipSuccess;
    }
    // The scratch of the three sums: [kBackdropGradBlocks][3] partials, then the [3] results.
    hipError_t sums(double** partials, double** out)
    {
        if (!sums_) S2D_TRY(sums_.alloc((size_t)(kBackdropGradBlocks + 1) * 3));
        *partials = sums_;
        *out = sums_ + (size_t)kBackdropGradBlocks * 3;
        return hipSuccess;
    }

private:
    hipError_t reserve_throughput(size_t pixels) { return throughput_ ? hipSuccess : throughput_.alloc(pixels); }

    Kind kind_ = None;
    BackdropArgs args_;
    DevBuf<float> throughput_; // [W * H], fp32 whatever the images are
    DevBuf<float4> plane_;     // [W * H]: the context's copy of a plane backdrop
    DevBuf<double> sums_;
};

} // namespace s2d
