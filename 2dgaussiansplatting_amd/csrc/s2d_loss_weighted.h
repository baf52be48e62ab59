// s2d_loss_weighted.h -- the image losses under a per-pixel weight plane (include/splat2d_weights.h):
// launch declarations of s2d_loss_weighted.hip and the owner of what a plane brings to a context.
//
//   L_omega = sum over pixels p of omega(p) * sum over channels of  w_mse * 1/2 * d^2 + w_l1 * |d| + w_dssim * (1 - s)
// The kernels are the bodies of s2d_loss.hip's (s2d_loss_kernels.h) with one multiply by omega per stored map value and per
// pointwise term, and a fourth sum: a plane of ones gives the unweighted kernels' bytes, gradient image and totals.
#pragma once

#include "s2d_loss.h"

namespace s2d {

// One weighted loss pass.  base: as for launch_loss, but base.partial and base.out3 are not the unweighted pass's:
// partial4 holds kWeightedTerms x slots doubles, out4 the four totals; base.out3 (the slot of the unweighted ring, so that
// whoever reads it finds the squared error where it always is) receives totals 0, 2 and 3.
struct WeightedLossArgs {
    LossArgs base;
    const float* omega = nullptr; // W * H
    double* partial4 = nullptr;
    double* out4 = nullptr;
};
hipError_t launch_loss_weighted(const WeightedLossArgs& a, hipStream_t stream);

// Is `plane` (pixels floats, device memory) a weight plane, and what is its sum?  partial: one double pair per 1024 pixels;
// out2[0] = the sum of the values (doubles, a fixed order), out2[1] = how many of them are NaN, infinite or negative.
inline size_t weight_check_slots(size_t pixels) { return (pixels + 1023) / 1024; }
hipError_t launch_weight_check(const float* plane, size_t pixels, double* partial, double* out2, hipStream_t stream);

// What a plane brings to a context: the plane itself, and the ring of the four totals of every iteration beside LossTrace's
// (same slots, same capacity).  Everything is allocated by the first plane.
class S2D_LOCAL PixelWeights {
public:
    TermRing ring{kWeightedTerms};
    bool set() const { return set_; }
    double sum() const { return set_ ? sum_ : 0.0; }
    const float* plane() const { return plane_; }

    // A buffer for a candidate plane and the scratch of its check.  The candidate becomes the plane with adopt(), and only then.
    hipError_t candidate(size_t pixels, float** plane, double** partial, double** out2)
    {
        S2D_TRY(candidate_.alloc(pixels));
        S2D_TRY(check_.reserve(2 * weight_check_slots(pixels) + 2));
        *plane = candidate_, *partial = check_, *out2 = check_ + 2 * weight_check_slots(pixels);
        return hipSuccess;
    }
    hipError_t adopt(int W, int H, double sum, hipStream_t stream)
    {
        S2D_TRY(ring.ensure(W, H, stream));
        plane_ = std::move(candidate_); // (the old plane goes with the candidate's owner: no stream uses it, the check was waited for)
        candidate_.release();
        sum_ = sum, set_ = true;
        return hipSuccess;
    }
    void discard_candidate() { candidate_.release(); }
    void clear()
    {
        plane_.release();
        set_ = false;
    }

private:
    DevBuf<float> plane_, candidate_;
    DevBuf<double> check_;
    double sum_ = 0.0;
    bool set_ = false;
};

} // namespace s2d
