// s2d_loss.h -- image losses formed on the device beside the reference's squared error (include/splat2d.h, s2d_loss_*;
// DESIGN.md section 13): launch declarations of s2d_loss.hip and the owner of what a loss pass leaves behind.
//
//   L = sum over pixels p and channels c of  w_mse * 1/2 * d^2 + w_l1 * |d| + w_dssim * (1 - s),   d = image0 - imageRef,
//   s the SSIM index under the separable 11-tap Gaussian window (sigma 1.5), zero padding of 5, C1 = 0.01^2, C2 = 0.03^2.
// A term whose weight is 0 is neither evaluated nor added: with (1, 0, 0) the gradient image is image0 - imageRef, the
// subtraction of main.cpp:616, bit for bit.
#pragma once

#include "s2d_device.h"
#include "s2d_owned.h"

namespace s2d {

constexpr int kLossTile = 32;   // pixels per edge of a loss tile (one 256-thread workgroup, 4 pixels per thread)
constexpr int kLossRadius = 5;  // the window reaches 5 pixels to every side
constexpr int kLossTaps = 2 * kLossRadius + 1;
constexpr int kLossMapPlanes = 9; // per channel: d(1-s)/d(mu_x) (total), d/d(w*x^2), d/d(w*xy); planar, one float per pixel each

struct LossWindow {
    float g[kLossTaps]; // exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in double, rounded to fp32
};

// One loss pass over the whole image.  partial: 3 x slots doubles (squared error on the reference's 255 scale, sum |d|,
// sum (1 - s)), slots = loss_slots(W, H); out3: the three totals; sqerr_out (may be null): the squared error once more, into
// the iteration's slot of the squared-error ring.
struct LossArgs {
    const void* image0 = nullptr;    // RGBA32F, or 4 x fp16 with half_images
    const void* image_ref = nullptr;
    bool half_images = false;
    int W = 0, H = 0;
    float w_mse = 0.0f, w_l1 = 0.0f, w_dssim = 0.0f;
    float* maps = nullptr;           // [kLossMapPlanes][W * H], only with w_dssim > 0
    float4* dimage = nullptr;        // dL/d(image0), RGBA32F, .w = 0
    double* partial = nullptr;
    double* out3 = nullptr;
    double* sqerr_out = nullptr;
    const DeviceStatus* status = nullptr;
    int iteration = 0;
};
inline int loss_slots(int W, int H) { return ((W + kLossTile - 1) / kLossTile) * ((H + kLossTile - 1) / kLossTile); }
hipError_t launch_loss(const LossArgs& a, hipStream_t stream);
const LossWindow& loss_window(); // the one window of every loss pass, built on first use (s2d_loss.hip)

// The totals of a pass: kLossTerms of them (squared error on the 255 scale, |d|, 1 - s), or under a weight plane
// (s2d_loss_weighted.h) kWeightedTerms: the squared error unweighted, then omega * that, omega * |d|, omega * (1 - s).
constexpr int kLossTerms = 3, kWeightedTerms = 4;

// Per-tile partial sums of `terms` terms, and their totals of every iteration in a ring beside the squared-error ring (slot
// iteration % kCapacity), plus one slot for a pass that belongs to no iteration (s2d_loss_image_grads_device).  Allocated by
// the first ensure().
class S2D_LOCAL TermRing {
public:
    static constexpr int kCapacity = 1 << 16;
    static constexpr int kEvalSlot = kCapacity; // of the pass that formed a gradient image alone
    static int slot_of(int iteration) { return iteration % kCapacity; }

    explicit TermRing(int terms) : terms_((size_t)terms) {}
    int terms() const { return (int)terms_; }
    hipError_t ensure(int W, int H, hipStream_t stream)
    {
        stream_ = stream;
        if (ring_) return hipSuccess;
        hipError_t e = partial_.alloc(terms_ * (size_t)loss_slots(W, H));
        if (e == hipSuccess) e = ring_.alloc(terms_ * (kCapacity + 1));
        if (e == hipSuccess) e = hipMemsetAsync(ring_, 0, terms_ * (kCapacity + 1) * sizeof(double), stream);
        return e;
    }
    double* partial() const { return partial_; }
    double* slot(int s) const { return ring_ + terms_ * (size_t)s; }
    // The totals of the iterations [first, first + count) -> out (terms() doubles each), queued.
    hipError_t read(int first, int count, double* out) const
    {
        for (int got = 0; got < count;) {
            const int s = slot_of(first + got), run = std::min(count - got, kCapacity - s);
            const hipError_t e = hipMemcpyAsync(out + terms_ * got, slot(s), terms_ * run * sizeof(double), hipMemcpyDeviceToHost, stream_);
            if (e != hipSuccess) return e;
            got += run;
        }
        return hipSuccess;
    }

private:
    const size_t terms_;
    hipStream_t stream_ = nullptr;
    DevBuf<double> partial_, ring_;
};

// What the loss passes of a context leave: the ring of the three totals, and which pass was the last.
class S2D_LOCAL LossTrace {
public:
    TermRing ring{kLossTerms};
    // A pass has been queued into slot `s` with these weights: what s2d_loss_get reports.
    void record(int s, float w_mse, float w_l1, float w_dssim) { last_ = s, w_[0] = w_mse, w_[1] = w_l1, w_[2] = w_dssim; }
    int last_slot() const { return last_; } // -1: no loss pass yet
    const float* last_weights() const { return w_; }

private:
    int last_ = -1;
    float w_[3] = {0.0f, 0.0f, 0.0f};
};

} // namespace s2d
