/* splat2d_weights.h -- a per-pixel weight plane for the losses and the step: a context that owns a plane
 * omega (height x width fp32, finite, >= 0, not all zero) trains on
 *
 *   L_omega = sum_p omega(p) * sum_c [ w_mse * 1/2 * d^2 + w_l1 * |d| + w_dssim * (1 - s_c(p)) ],   d = image0 - imageRef,
 *
 * s the SSIM index of splat2d.h ("image losses").  A mask (omega in {0, 1}) keeps a region from attracting splats, a plane above
 * 1 somewhere makes that region matter more.  It adds four entry points and one structure to the same library and no
 * configuration flag: the plane is state of an ordinary context, and a context without one behaves exactly as it always did.
 *
 *   s2d_set_pixel_weights(ctx, mask);              height * width floats in host memory
 *   s2d_step(ctx, 500, 0, mse);                    trains on sum omega * d^2 / 2; mse stays the plain one
 *   s2d_set_pixel_weights(ctx, NULL);              plain again, fused launch included
 *
 * The gradient, with the three derivative maps A, B, Cm of DESIGN.md section 13 taken at the window's centre:
 *   g(p) = omega(p) * (w_mse * d + w_l1 * sign d) + w_dssim * [ (w*(omega A))(p) + 2 x(p) (w*(omega B))(p) + y(p) (w*(omega Cm))(p) ]
 * In fp32 the weighted kernels do what the unweighted ones do plus one multiply by omega per stored map value and per
 * pointwise term, so a plane of ones gives the bytes of a context without a plane, and a plane that is 2^k everywhere
 * gives 2^k times its gradient image, exactly.
 *
 * While a plane is set
 *   s2d_loss_image_grads_device, s2d_loss_backward and s2d_step_loss differentiate L_omega; s2d_loss_get reports l1, dssim and
 *     total of L_omega (each weighted sum divided by 3 * H * W) and loss_out of s2d_step_loss the same total; mse, s2d_get_mse and
 *     the squared-error trace stay the UNWEIGHTED squared error, the reference's number;
 *   s2d_backward, s2d_forward_backward and s2d_step run the separate launches (as over a backdrop) with the weighted loss pass
 *     of weights (1, 0, 0) between the two walks: they train on what the plane says instead of ignoring it;
 *   the caller's own upstream gradients (s2d_backward_image_grads, s2d_view_backward_device without S2D_VIEW_BWD_FROM_TARGET,
 *     s2d_backdrop_grads with an upstream) are untouched: the loss is the caller's;
 *   S2D_E_INVALID, before any device work, with a message that names s2d_set_pixel_weights(ctx, NULL): s2d_step_view,
 *     s2d_view_backward_device and s2d_view_grads with S2D_VIEW_BWD_FROM_TARGET (the plane is not resampled to a view),
 *     s2d_backdrop_grads with a NULL upstream, and whatever the loss passes refuse (s2d_halo_commit's held set).
 * The importance map S2D_SEED_ERROR stays unweighted; a caller passes a map of their own with S2D_SEED_CALLER.
 * Setting, replacing or removing a plane invalidates nothing but the terms of the last loss pass (s2d_loss_get is S2D_E_STATE
 * until the next one): image0, the gradients, the projection and the lists stand.
 * The multi-device handle has no plane (its contexts own row slabs), and a checkpoint of the host program does not carry it.
 */
#ifndef SPLAT2D_WEIGHTS_H
#define SPLAT2D_WEIGHTS_H

#include "splat2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The terms of the last loss pass under a plane.  mse, l1, dssim: the sums over pixels and channels of omega * d^2, omega * |d|
 * and omega * (1 - s), each divided by 3 * H * W (NOT by the sum of the weights: weight_sum is there for whoever wants that
 * mean); total = w_mse * 1/2 * mse + w_l1 * l1 + w_dssim * dssim = L_omega / (3 H W).  A term whose weight was 0 is NaN, as in
 * s2d_loss_terms -- mse is always formed. */
typedef struct s2d_weighted_terms {
    uint32_t struct_size; /* = sizeof(s2d_weighted_terms), set by the caller */
    uint32_t reserved;    /* 0 */
    double weight_sum;    /* sum of omega over the pixels */
    double mse, l1, dssim, total;
} s2d_weighted_terms;

/* The plane from HOST memory: height * width floats, row by row.  It is copied into a plane the context owns and checked
 * there by a kernel that also sums it (doubles, one fixed order); the call waits for that verdict.  NULL removes the plane.
 * S2D_E_INVALID: a value that is NaN, infinite or negative, or a plane of zeros -- the previous plane (or none) stays; a
 * context with S2D_CFG_COVERAGE or S2D_CFG_COUNT_PAIRS, a slab context, a context that holds a subset (s2d_halo_commit). */
int s2d_set_pixel_weights(s2d_ctx* ctx, const float* host_plane);

/* The same from DEVICE memory, 16-byte aligned; the caller's buffer may be reused when the call returns.  NULL removes the
 * plane.  Additionally S2D_E_INVALID for a misaligned pointer. */
int s2d_set_pixel_weights_device(s2d_ctx* ctx, const float* device_plane);

/* *set = 1 with a plane, 0 without; *weight_sum (may be NULL) its sum (0 without); host_plane_or_NULL receives the plane's
 * height * width floats (untouched without a plane). */
int s2d_get_pixel_weights(s2d_ctx* ctx, int32_t* set, double* weight_sum, float* host_plane_or_NULL);

/* The weighted terms of the last loss pass.  S2D_E_INVALID without a plane or with a wrong struct_size; S2D_E_STATE before
 * a loss pass under the current plane. */
int s2d_weighted_loss_get(s2d_ctx* ctx, s2d_weighted_terms* out);

#ifdef __cplusplus
}
#endif
#endif /* SPLAT2D_WEIGHTS_H */
