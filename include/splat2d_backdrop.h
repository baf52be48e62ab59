/* splat2d_backdrop.h -- a backdrop behind the splats: the context composites what it draws over a
 * constant colour or over an image of its own size, and trains the splats through that composite.  It adds five entry points to
 * the same library, no structure and no configuration flag: a backdrop is state of an ordinary context.
 *
 *   const float white[3] = { 1.f, 1.f, 1.f };
 *   s2d_set_backdrop(ctx, white);                  from now on image0 = C + T_final * white
 *   s2d_step(ctx, 500, 0, mse);                    the fit leaves the light ground to the backdrop
 *
 * For every pixel and colour channel, in fp32, one multiply and then one add, never contracted:
 *   image0.c = C.c + (T_final * B.c)
 * C and T_final are the colour and the throughput the reference's loop (main.cpp:414-536) leaves for the pixel; image0.w stays 1.
 * A context with S2D_CFG_FP16_IMAGES forms the sum in fp32 and rounds it at the store, like the colours.  A backdrop of (0, 0, 0)
 * therefore gives the bytes of a context without one.  Every other pass of an iteration works on image0 as stored: the backward
 * walk forms S = image0 - running (main.cpp:627), which then carries the backdrop's share, so its gradients are those of the
 * composite; the squared error, the native losses and the density statistics are the composite's too.
 *
 * While a backdrop is set s2d_step, s2d_forward_backward and s2d_step_loss queue the forward and the backward walk as separate
 * launches: image0 is stored every iteration and S2D_FB_SKIP_IMAGE has no effect.
 * Setting, replacing or removing a backdrop makes image0 and the gradients stale; the projection and the tile lists stand.
 *
 * Not available, S2D_E_INVALID from the two setters before any device work: a context with S2D_CFG_COVERAGE, S2D_CFG_COUNT_PAIRS,
 * S2D_CFG_EXACT_EXP or S2D_CFG_REFERENCE_ORDER, a slab context, a context that holds a subset (s2d_halo_commit).
 * While a backdrop is set: s2d_view_backward_device, s2d_view_grads, s2d_step_view (splat2d_coarse.h), s2d_halo_masks and
 * s2d_halo_commit are S2D_E_INVALID (the view gradient kernels form the final colour themselves, without the backdrop);
 * s2d_render_view, s2d_render_view_device are S2D_E_INVALID over a plane (it would have to be resampled) and draw over a constant:
 * the backdrop is added per sample before the resolve, so the view is what a context of the raster grid's size would draw,
 * resolved, and the identity view is image0 byte for byte.  A scene beyond the pair budget of one set of lists (index-range
 * rendering) is S2D_E_NOMEM at s2d_forward.  A refused call leaves gradients, image0 and the iteration counter as they were.
 * The multi-device handle has no backdrop, and a checkpoint of the host program does not carry it.
 */
#ifndef SPLAT2D_BACKDROP_H
#define SPLAT2D_BACKDROP_H

#include "splat2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A constant backdrop (r, g, b); NULL removes the backdrop of either kind: the context is plain again, fused launch included.
 * S2D_E_INVALID: a value that is not finite; the contexts listed above. */
int s2d_set_backdrop(s2d_ctx* ctx, const float rgb[3]);

/* A plane backdrop: height x width RGBA32F in DEVICE memory, 16-byte aligned, .w ignored.  The plane is copied, on the context's
 * stream, into a buffer the context owns: the caller's may be reused once the stream has passed the copy.
 * S2D_E_INVALID: a NULL or misaligned pointer; the contexts listed above. */
int s2d_set_backdrop_device(s2d_ctx* ctx, const float* rgba32f_rows_device);

/* *kind = 0 (none), 1 (constant) or 2 (plane); rgb (may be NULL) receives the constant, zeros otherwise. */
int s2d_get_backdrop(s2d_ctx* ctx, int* kind, float rgb[3]);

/* T_final of the last forward pass: height x width floats into DEVICE memory, queued on the context's stream.  Available only
 * while a backdrop is set (S2D_E_INVALID otherwise; a black backdrop is how a caller asks for the plane alone), and only behind a
 * forward pass on the current parameters and backdrop (S2D_E_STATE otherwise). */
int s2d_throughput_device(s2d_ctx* ctx, float* plane_device);

/* dL/dB from dL/d(image0).  g = upstream_rows_device (height x width RGBA32F in device memory, 16-byte aligned, .w ignored) or,
 * with NULL, image0 - target as the backward walk forms it.  Per pixel and channel the term is t_c = T_final * g_c, one fp32
 * multiply.  dplane_device (may be NULL; height x width RGBA32F, 16-byte aligned) receives (t_r, t_g, t_b, 0): the gradient of a
 * plane.  rgb_out (may be NULL; host memory) receives the three sums of the terms over the image, the gradient of a constant:
 * each term converted to double, added in a fixed order without atomics -- two calls return the same bytes.  Waits for the
 * stream when rgb_out is given.  S2D_E_INVALID without a backdrop or with a misaligned pointer; S2D_E_STATE without a forward
 * pass on the current parameters and backdrop or, with a NULL upstream, without a target. */
int s2d_backdrop_grads(s2d_ctx* ctx, const float* upstream_rows_device, float* dplane_device, double rgb_out[3]);

#ifdef __cplusplus
}
#endif
#endif /* SPLAT2D_BACKDROP_H */
