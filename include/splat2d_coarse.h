/* splat2d_coarse.h -- coarse-to-fine fitting on top of the views of splat2d.h: the context's target seen
 * through a view's window, and whole training iterations at the view's size.  It adds two entry points to the same library
 * and no structure: a view is described by the s2d_view_config of splat2d.h.
 *
 *   s2d_view_config v = { sizeof v, (W + 3) / 4, (H + 3) / 4, 0.f, 0.f, 0.25f, 0.f, 1, S2D_VIEW_RGBA32F };
 *   s2d_step_view(ctx, &v, NULL, 100, 0, mse);     100 quarter-size iterations against the library's own small target
 *   s2d_view_release(ctx);
 *   s2d_step(ctx, 400, 0, mse + 100);              and on at full size
 */
#ifndef SPLAT2D_COARSE_H
#define SPLAT2D_COARSE_H

#include "splat2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The context's target seen through the view's window: out_height x out_width RGBA32F in DEVICE memory, 16-byte aligned, queued
 * on the context's stream.  An area (box) resample, exact and order-defined, all in fp32, one operation at a time:
 *   output pixel (i, j) covers the source rectangle [x0, x1) x [y0, y1),
 *     x0 = origin_x + (float)i / zoom,  x1 = origin_x + (float)(i + 1) / zoom,  y alike with j and origin_y;
 *   source pixel c covers [c, c + 1) and has the weight w(c) = min(x1, (float)(c + 1)) - max(x0, (float)c), its overlap length;
 *   columns floor(x0) .. ceil(x1) - 1 and rows floor(y0) .. ceil(y1) - 1 are visited, those outside the image left out: a source
 *   pixel outside the image counts as 0, the black the views draw on;
 *   value = (sum over rows, ascending, of wy * (sum over columns, ascending, of wx * t)) * (zoom * zoom), each sum starting from
 *   0.0f, for all four channels alike.
 * A context with S2D_CFG_FP16_IMAGES reads the fp16 target it stores, converted to fp32.  Of the configuration only out_width,
 * out_height, origin and zoom enter: filter_var and samples describe how the SPLATS are drawn and do not touch the target.
 * At zoom 1/2 or 1/4 with an integer origin this is the plain mean of the 2 x 2 or 4 x 4 block.
 * One thread forms an output pixel and visits the (1 / zoom)^2 source pixels under it one after the other: cheap at the zooms of
 * a schedule, a whole kernel's work in a single lane at very small ones, so zoom < 1/256 is refused.
 * S2D_E_INVALID, before any device work: everything s2d_step_view refuses for the configuration or the context (below), zoom
 * < 1/256, a NULL or misaligned pointer.  The target need not have been set: a context's target starts out black. */
int s2d_view_target_device(s2d_ctx* ctx, const s2d_view_config* cfg, float* out_device);

/* `iters` iterations of: view of the current splats -> view - target -> gradients -> s2d_adam_step.  The counterpart of s2d_step
 * at a view's size.  Per iteration, on the context's stream: the view's records, projection and lists (the one host wait of a
 * view: the pair count), ONE kernel that walks every tile forward and backward as s2d_view_backward_device's does and also
 * leaves the tile's squared error, on a deterministic context the gather, the sum of the tile errors in a fixed order, the
 * adjoint of the record transform into the gradient buffer, and the Adam launch of s2d_adam_step: the iteration count and the
 * beta powers advance, and the optimiser controls, the frozen mask and the alive set act as always.  The gradients are, byte
 * for byte, those of s2d_view_backward_device(S2D_VIEW_BWD_FROM_TARGET) followed by s2d_adam_step.
 *
 * target_device: out_height x out_width RGBA32F in device memory, 16-byte aligned, .w ignored; or NULL = the library's own
 * s2d_view_target_device of this configuration, which it keeps and rebuilds when the window changes or s2d_set_target* replaced
 * the target it was made from.
 * mse_out (may be NULL) receives iters doubles, main.cpp:796-805 at the view's size, evaluated BEFORE that iteration's step: the
 * sum over output pixels of |(view - target).rgb * 255|^2, a float per pixel, added up in double in a fixed order, divided by
 * out_height * out_width * 3.
 * flags: S2D_STEP_OPTIMIZE_OPACITY; anything else is S2D_E_INVALID.  iters == 0 does nothing.
 * A parameter that went non-finite: S2D_E_NONFINITE and NaN in the rest of mse_out, as for s2d_step.
 *
 * image0, the training lists and their rebuild counters, s2d_get_mse and the squared-error ring keep what they had (the
 * projection is stale after an Adam step, as ever).  The buffers of the call (tile errors, the library's own target) are the
 * view's: s2d_view_release and s2d_destroy free them.
 *
 * S2D_E_INVALID, before any device work: everything s2d_view_backward_device is refused for (a context with S2D_CFG_COVERAGE,
 * S2D_CFG_COUNT_PAIRS or S2D_CFG_REFERENCE_ORDER, a slab context or a held set, format != S2D_VIEW_RGBA32F); unknown flags;
 * iters < 0; a misaligned pointer; with a NULL target, zoom < 1/256 (s2d_view_target_device).  S2D_E_NOMEM as for a view (the pair budget S2D_CHUNK_PAIRS).  After a refusal the context
 * trains on unchanged. */
int s2d_step_view(s2d_ctx* ctx, const s2d_view_config* cfg, const float* target_device, int32_t iters, uint32_t flags, double* mse_out);

#ifdef __cplusplus
}
#endif
#endif /* SPLAT2D_COARSE_H */
