/*
 * splat2d.h -- C ABI of the MI355X-native 2D Gaussian splatting trainer.
 *
 * The reference (Ushio/2dGaussianSplatting, /root/reference/main.cpp) has no
 * plugin / FFI interface: the forward rasteriser, the analytic backward pass and
 * the Adam step are inline loops inside main()'s frame loop (main.cpp:334-851)
 * that communicate through main()'s locals.  This boundary is therefore drawn
 * around the locals those three passes own:
 *
 *   std::vector<Splat> splats          main.cpp:272      <-> s2d_set_splats / s2d_get_splats
 *   std::vector<SplatAdam> splatAdams  main.cpp:276      <-> s2d_set_adam / s2d_get_adam
 *   float beta1t, beta2t               main.cpp:274-275  <-> s2d_set_adam / s2d_get_adam
 *   int iterations                     main.cpp:278      <-> s2d_set_adam / s2d_get_adam
 *   Image2DRGBA32 imageRef             main.cpp:254-259  <-> s2d_set_target
 *   Image2DRGBA32 image0               main.cpp:310      <-> s2d_get_image
 *   std::vector<Splat> dSplats         main.cpp:550      <-> s2d_get_grads
 *   bool optimizeOpacity               main.cpp:317      <-> S2D_STEP_OPTIMIZE_OPACITY
 *   float trainingRate                 main.cpp:715      <-> s2d_config.training_rate
 *   abort() on non-finite params       main.cpp:752-785  <-> status S2D_E_NONFINITE
 *
 * Conventions: plain C, opaque handle, int status returns (0 = OK), no exceptions
 * or aborts across the boundary.  All `const T*` / `T*` arguments are HOST pointers
 * owned by the caller unless the name says `_device`.  A context is driven by one
 * host thread; it owns its device memory; work is queued on its HIP stream and
 * host-visible results are complete when the call that returns them returns.
 *
 * There is NO CPU fallback: every entry point that computes runs hand-written
 * HIP kernels for gfx950 and fails with S2D_E_HIP when no device is usable.
 */
#ifndef SPLAT2D_H
#define SPLAT2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct that crosses the boundary changes layout or an entry point changes meaning; added entry points
 * alone do not bump it.  s2d_abi_version() returns the value the LIBRARY was built with: a caller compares it with this
 * macro before anything else (the Python binding does, load_library()).
 *   2: s2d_stats starts with struct_size (round 2 had grown the struct in place under version 1). */
#define S2D_ABI_VERSION 2

/* == struct Splat, main.cpp:85-93 (vec2 pos; float sx, sy, rot; vec3 color; float opacity): 36 bytes.
 * Also the gradient record (dSplats, main.cpp:550). */
typedef struct s2d_splat {
    float pos[2];
    float sx, sy, rot;
    float color[3];
    float opacity;
} s2d_splat;

/* == struct Adam, main.cpp:139-157 */
typedef struct s2d_adam { float m, v; } s2d_adam;

/* == struct SplatAdam, main.cpp:158-166: 72 bytes */
typedef struct s2d_splat_adam {
    s2d_adam pos[2];
    s2d_adam sx, sy, rot;
    s2d_adam color[3];
    s2d_adam opacity;
} s2d_splat_adam;

typedef enum s2d_status {
    S2D_OK = 0,
    S2D_E_INVALID = 1,    /* bad argument / bad config */
    S2D_E_HIP = 2,        /* HIP runtime error or no usable gfx950 device (see s2d_last_error) */
    S2D_E_NONFINITE = 3,  /* a parameter the reference checks (main.cpp:752-785) became non-finite */
    S2D_E_NOMEM = 4,
    S2D_E_STATE = 5       /* call order violated (e.g. backward before forward, no target set) */
} s2d_status;

/* s2d_step / s2d_adam_step flags */
#define S2D_STEP_OPTIMIZE_OPACITY 0x1u /* the "Optimize opacity" checkbox, main.cpp:317, :735-738, :825 */
#define S2D_STEP_DENSITY_STATS 0x2u    /* s2d_step only: these iterations run as s2d_forward, s2d_backward with
                                        * S2D_BWD_DENSITY_STATS, s2d_adam_step instead of the fused launch -- the same
                                        * results (bitwise with S2D_CFG_DETERMINISTIC), one statistics pass per iteration.
                                        * Refused like S2D_BWD_DENSITY_STATS. */

/* s2d_backward / s2d_forward_backward flags */
#define S2D_BWD_SKIP_OPACITY_GRAD 0x1u /* leave dSplats.opacity at zero.  The reference always accumulates it
                                        * (main.cpp:704) but reads it only when "Optimize opacity" is on (main.cpp:735):
                                        * a caller whose next s2d_adam_step runs without S2D_STEP_OPTIMIZE_OPACITY
                                        * may skip it.  s2d_step does so by itself. */
#define S2D_BWD_DENSITY_STATS 0x4u     /* s2d_backward, s2d_backward_image_grads: the pass also ACCUMULATES the density
                                        * statistics of every splat (s2d_density, below) and counts one statistics pass; the
                                        * gradients come out as without the flag.  S2D_E_INVALID for s2d_forward_backward
                                        * (the fused launch has no such variant) and for S2D_CFG_COUNT_PAIRS,
                                        * S2D_CFG_EXACT_EXP and S2D_CFG_REFERENCE_ORDER contexts; S2D_E_NOMEM for a scene
                                        * rendered by index ranges (see s2d_forward). */
#define S2D_FB_SKIP_IMAGE 0x2u         /* s2d_forward_backward only: do not store image0 (the backward walk takes the final
                                        * colours from registers); s2d_get_image then returns an older frame.  For training
                                        * loops that never look at it. */

/* s2d_config.flags */
#define S2D_CFG_COUNT_PAIRS 0x1u   /* count visited / active pixel-splat pairs in the raster kernels (diagnostic) */
#define S2D_CFG_FP16_IMAGES 0x2u   /* BASELINE configs[4] "fp16 color / fp32 grads": the framebuffer and the target are
                                    * held in HBM as 4 x fp16 per pixel (round to nearest even); all arithmetic, the
                                    * gradients and the optimiser stay fp32.  Images still cross this ABI as RGBA32F.
                                    * Not the reference's arithmetic: results equal the reference run with imageRef and
                                    * image0 rounded to fp16 (tests/test_gpu_parity.py::test_fp16_images_*). */
#define S2D_CFG_DETERMINISTIC 0x4u /* bitwise reproducible gradients: tiles store their per-splat partial sums into
                                    * private slots and a gather pass adds them in a fixed order, instead of float
                                    * atomics whose arrival order varies from run to run (the forward pass is
                                    * deterministic either way).  About a sixth slower at 4096^2 / 10^6 splats. */
#define S2D_CFG_EXACT_EXP 0x8u     /* validation mode: exp_approx returns expf(x), the switch the reference keeps at
                                    * main.cpp:51 "for numerical varidation".  The analytic gradients (main.cpp:639-704)
                                    * are those of the true exponential, so in this mode the backward pass is the
                                    * derivative of the forward pass and a finite-difference check closes
                                    * (tests/test_fd_end_to_end.py).  The expf has the bits of glibc's (the reference built
                                    * with g++ on x86-64), so image0 is the reference's byte for byte in this mode too.
                                    * Not combinable with S2D_CFG_COUNT_PAIRS / S2D_CFG_FP16_IMAGES. */
#define S2D_CFG_ADAM_FP32 0x10u    /* Adam::optimize (main.cpp:155) with the quotient and subtraction in fp32, as the
                                    * reference's own MSVC build evaluates the unqualified `sqrt` (float overload).
                                    * Default: the double-precision quotient of a g++/clang++ build, which is what the
                                    * known-answer vectors pin.  The two differ by <= 1 ulp
                                    * of the parameter + ~3 ulp of the update per step; 100-iteration MSE traces by 2e-5
                                    * (tests/test_oracle_kat.py). */

#define S2D_CFG_GENERIC_BINNING 0x20u /* diagnostic: build the tile lists with the generic builder (all (tile, splat) pairs
                                    * radix-sorted by tile) even where the two-level one applies (images of up to 512 tile
                                    * columns, csrc/s2d_tilelists.hip).  Same lists either way; wider images always use it. */
#define S2D_CFG_REFERENCE_ORDER 0x40u /* validation mode: dSplats, the updated splats / splatAdams and the MSE come out
                                    * bytes-equal to the reference's.  Every backward pass (s2d_backward, s2d_forward_backward,
                                    * s2d_step, s2d_backward_image_grads) evaluates the nine addends of each (splat, pixel)
                                    * with the reference's own expressions (main.cpp:618-704), stores them per (tile, splat)
                                    * pair, and adds each splat's in ONE fp32 chain in the order of main.cpp:576-598 (pixel
                                    * rows ascending, columns ascending); the squared error is the row-major double chain of
                                    * main.cpp:796-805.  Only speed and memory differ from the reference: 9 KiB of scratch
                                    * per pair of capacity, at most S2D_REFERENCE_ORDER_MAX_BYTES (environment, read at
                                    * s2d_create; default 32 GiB), S2D_E_NOMEM beyond.  With S2D_CFG_DETERMINISTIC the
                                    * result is that of this flag alone.  Not combinable with S2D_CFG_COUNT_PAIRS /
                                    * S2D_CFG_FP16_IMAGES, s2d_multi_create or slab ownership (s2d_halo_commit with masks):
                                    * S2D_E_INVALID; no index-range rendering (see s2d_forward). */
#define S2D_CFG_COVERAGE 0x80u     /* coverage channel: every pixel carries a fourth running value
                                    * ca, 0 at the start and ca += T * alpha beside main.cpp:529-531 -- the colour sum of a
                                    * channel whose colour is 1 in every splat, 1 - T_final up to rounding.  s2d_forward stores
                                    * image0 = (r, g, b, ca); the .w of the target (s2d_set_target) is the alpha to fit and the
                                    * loss of s2d_backward is the half squared error over four channels; the .w of the image
                                    * gradient of s2d_backward_image_grads is dL/d(ca); a view's .w (alpha byte) is ca resolved
                                    * (quantised) like the colours.  .rgb stays premultiplied colour on black, and the squared
                                    * error (trace ring, s2d_get_mse) the three-channel quantity.  s2d_forward_backward and
                                    * s2d_step queue the separate launches and store image0 every iteration (S2D_FB_SKIP_IMAGE
                                    * has no effect).  S2D_E_INVALID: together with S2D_CFG_COUNT_PAIRS, S2D_CFG_EXACT_EXP,
                                    * S2D_CFG_REFERENCE_ORDER or a row slab at s2d_create; s2d_multi_create; s2d_halo_masks
                                    * and s2d_halo_commit; S2D_BWD_DENSITY_STATS / S2D_STEP_DENSITY_STATS; s2d_loss_backward,
                                    * s2d_step_loss, s2d_loss_image_grads_device; s2d_view_backward_device and s2d_view_grads.
                                    * S2D_E_NOMEM for a scene that would be rendered by index ranges (see s2d_forward). */

typedef struct s2d_config {
    uint32_t struct_size;   /* = sizeof(s2d_config) */
    int32_t width, height;  /* imageRef.width(), .height() (main.cpp:254) */
    int32_t n_splats;       /* NSplat (main.cpp:271) */
    int32_t device;         /* HIP device ordinal */
    /* Row slab [row_begin, row_end) of the image this context rasterises.
     * 0,0 = the whole image.  row_begin must be a multiple of 16 (the tile height). */
    int32_t row_begin, row_end;
    float training_rate;    /* 0 -> 0.05f (main.cpp:715) */
    uint32_t flags;         /* S2D_CFG_* */
    /* Tile lists may be re-used across iterations: they are built from tile rectangles inflated by
     * rebin_margin + |sx - sy| pixels, and every iteration a device-side check forces a rebuild BEFORE the raster runs if
     * any splat's exact rectangle left its binned one, so results do not depend on these two knobs.
     * rebin_interval: 0 -> library default (rebuild only when the check fires); 1 -> rebuild every iteration;
     * K > 1 -> additionally rebuild at least every K iterations.  rebin_margin: 0 -> default (2 pixels). */
    int32_t rebin_interval;
    float rebin_margin;
    void* stream;           /* hipStream_t to queue work on; NULL -> the context creates its own */
} s2d_config;

typedef struct s2d_stats {
    uint32_t struct_size;      /* IN: sizeof(s2d_stats) as the caller was compiled; s2d_get_stats writes no more than that */
    uint32_t reserved;
    uint64_t pairs_binned;     /* (tile, splat) pairs in the current tile lists (index-range rendering: of the range built last) */
    uint64_t pairs_capacity;
    uint64_t rebins;           /* times the tile lists were rebuilt */
    uint64_t fwd_visited, fwd_active; /* S2D_CFG_COUNT_PAIRS: pairs inside the reference's x/y ranges, and those with T >= 1/256 */
    uint64_t bwd_visited, bwd_active;
    uint64_t fwd_staged, bwd_staged;  /* list entries the raster kernels actually staged (after tile retirement) */
    uint64_t fwd_wave_execs, bwd_wave_execs; /* (wave, entry) pairs whose blend body ran (>= 1 live lane covered) */
    uint64_t bwd_lane_hist[65];              /* ... of the backward pass, by number of active lanes (0..64) */
    int32_t iterations;        /* == `iterations`, main.cpp:278 */
    int32_t first_nonfinite_iteration; /* -1 if none */
    uint64_t fwd_staged_hit;   /* S2D_CFG_COUNT_PAIRS: staged entries that cover >= 1 pixel of their tile ... */
    uint64_t fwd_rows_hit;     /* ... and (staged entry, tile row) pairs with a non-empty column range (of 16 per entry) */
    uint64_t bwd_quadrant_execs; /* S2D_CFG_COUNT_PAIRS: bwd_wave_execs weighted by the number (1..4) of 4x4 quadrants of the
                                  * wave's 8x8 block that hold a live covered pixel */
} s2d_stats;

typedef struct s2d_ctx s2d_ctx;

int s2d_abi_version(void);

/* Allocates device state for (width, height, n_splats).  Splats are zero until s2d_init_splats / s2d_set_splats. */
int s2d_create(const s2d_config* cfg, s2d_ctx** out);
void s2d_destroy(s2d_ctx* ctx);

/* imageRef (main.cpp:254-259): width*height RGBA32F, row-major, .rgb in [0,1]; copied.  A slab context
 * (row_begin/row_end) is handed the same full-size buffer and uploads and keeps only its own rows: device memory for
 * imageRef and image0 is (row_end - row_begin) * width pixels each. */
int s2d_set_target(s2d_ctx* ctx, const float* rgba32f);
/* Fills imageRef on the device with ref(x,y) = (x/W, 1 - x/W, y/H, 1): the reference's commented generator
 * (main.cpp:261-267) plus a blue ramp, evaluated in fp32. */
int s2d_set_target_synthetic(s2d_ctx* ctx);

/* init(), main.cpp:280-305: pcg3d-seeded splats, Adam state zeroed, beta powers = 1, iterations = 0. */
int s2d_init_splats(s2d_ctx* ctx);
int s2d_set_splats(s2d_ctx* ctx, const s2d_splat* splats);
int s2d_get_splats(s2d_ctx* ctx, s2d_splat* splats);
/* Checkpointable optimiser state (main.cpp:274-278). */
int s2d_set_adam(s2d_ctx* ctx, const s2d_splat_adam* adams, float beta1t, float beta2t, int32_t iterations);
int s2d_get_adam(s2d_ctx* ctx, s2d_splat_adam* adams, float* beta1t, float* beta2t, int32_t* iterations);

/* Forward rasteriser, main.cpp:414-546 (rows of this context's slab).
 * No scene the reference's loops can run is refused for its size: the (tile, splat) pairs of the tile lists are addressed
 * with 32 bits, and a scene with more of them than S2D_CHUNK_PAIRS (environment, read at s2d_create; default 2^30) is
 * rendered by consecutive INDEX RANGES of the splats -- the lists of one range at a time, front to back like main.cpp:419
 * and :552, the per-pixel colour and throughput carried from range to range -- with the same bits as one set of lists
 * (forward, backward and s2d_step alike; only S2D_CFG_COUNT_PAIRS and S2D_CFG_REFERENCE_ORDER contexts answer S2D_E_NOMEM
 * there, the latter because its term scratch is addressed by the pairs of one set of lists). */
int s2d_forward(s2d_ctx* ctx);
/* image0 as uploaded at main.cpp:794: width*height RGBA32F, .w = 1 (S2D_CFG_COVERAGE: .w = coverage).  Rows outside the
 * slab are returned as 0. */
int s2d_get_image(s2d_ctx* ctx, float* rgba32f);
/* The slab's rows of image0 alone: (row_end - row_begin) * width RGBA32F, first row = row_begin (what a multi-GPU host
 * stitches together; s2d_get_image of a whole-image context returns the same bytes). */
int s2d_get_image_rows(s2d_ctx* ctx, float* rgba32f_rows);

/* Backward pass, main.cpp:548-712: accumulates this slab's contribution into the gradient buffer
 * (which s2d_adam_step / s2d_step re-zero after use, like main.cpp:550).  Needs s2d_forward first. */
int s2d_backward(s2d_ctx* ctx, uint32_t flags);
/* s2d_forward + s2d_backward in one kernel launch per tile (same results: a tile's backward walk needs only its own
 * pixels' final colours).  What s2d_step queues; for callers that put their own work between backward and Adam (the
 * multi-GPU exchange).  flags: S2D_BWD_SKIP_OPACITY_GRAD, S2D_FB_SKIP_IMAGE. */
int s2d_forward_backward(s2d_ctx* ctx, uint32_t flags);
int s2d_get_grads(s2d_ctx* ctx, s2d_splat* dsplats);

/* ---- the rasteriser as a building block: any loss on image0, formed by the caller on the device (INTEGRATION.md
 * section 5; torch_op.py wraps these three into a torch.autograd.Function) ---- */
/* Backward pass (main.cpp:548-712) with dL/d(image0) supplied by the caller instead of image0 - imageRef (main.cpp:616):
 * DEVICE pointer, (row_end - row_begin) * width RGBA32F, first row = row_begin, 16-byte aligned; .w ignored, or with
 * S2D_CFG_COVERAGE dL/d(coverage), which reaches position, scales, rotation and opacity but no colour.
 * Accumulates into the gradient buffer like s2d_backward; needs s2d_forward on the current parameters (S2D_E_STATE
 * otherwise, also after a fused launch with S2D_FB_SKIP_IMAGE); S2D_E_INVALID for a S2D_CFG_COUNT_PAIRS context.
 * flags: S2D_BWD_SKIP_OPACITY_GRAD.  Forms no squared error: the trace ring and s2d_get_mse keep what they had.
 * The values are not checked: a non-finite one reaches the gradients, and the finite guard of the next s2d_adam_step
 * judges the parameters as always. */
int s2d_backward_image_grads(s2d_ctx* ctx, const float* dimage_rows_device, uint32_t flags);
/* s2d_set_splats / s2d_get_image_rows with DEVICE pointers, queued on the context's stream, no host synchronisation.
 * s2d_set_splats_device keeps the tile lists (the containment check rebuilds them when a splat left its binned
 * rectangle) and the status word; the image buffer must be 16-byte aligned. */
int s2d_set_splats_device(s2d_ctx* ctx, const float* splats_device);     /* n_splats * 9 floats */
int s2d_get_image_rows_device(s2d_ctx* ctx, float* rgba32f_rows_device); /* always RGBA32F */

/* ---- density control (no counterpart in the reference, whose splat set is frozen at init(), main.cpp:280-305; DESIGN.md
 * section 12).  Two statistics per splat, gathered by the backward walk where the per-pixel addends exist:
 *   abs_dpos = sum over pixels of |dL_p/dpos.x|, |dL_p/dpos.y| -- the magnitudes of the addends of main.cpp:654-655, which no
 *              upstream gradient handed to s2d_backward_image_grads can produce (the sum of magnitudes is not linear in it);
 *   weight   = sum over pixels of T * alpha (main.cpp:618): how much of the image the splat is responsible for; a splat
 *              buried below the throughput cut-off (main.cpp:604) has 0 and receives no gradient at all.
 * Sums over the pixels of the context's slab and over the statistics passes since the last reset; every term is >= 0, so
 * the values of slab contexts add up to the whole image's.  The buffer exists from the first pass that asks for it. */
typedef struct s2d_density {
    float abs_dpos[2];
    float weight;
} s2d_density;
/* host[n_splats] and the number of accumulated passes (either may be NULL).  All zeros and 0 before any statistics pass.
 * s2d_init_splats resets the statistics; s2d_set_splats and s2d_set_splats_device do not (a caller that moves parameters
 * decides for itself). */
int s2d_density_get(s2d_ctx* ctx, s2d_density* host, int32_t* passes);
/* The same into DEVICE memory (n_splats * 3 floats), queued on the context's stream. */
int s2d_density_get_device(s2d_ctx* ctx, float* out_device, int32_t* passes);
int s2d_density_reset(s2d_ctx* ctx);
/* Moves up to max_moves STARVED splats (weight / passes < min_weight, the lowest first) onto halves of the splats with the
 * largest |abs_dpos| / passes: the donor's larger scale is divided by `shrink` (0 -> 1.6) and clamped to [1, 1024], the donor
 * moves half of that along the scale's axis one way, the starved row becomes a copy of it the other way, and the Adam moments
 * of both are zeroed; everything else, beta1t / beta2t / iterations included, is untouched (the exact rules:
 * csrc/s2d_density.h, deterministic, no random numbers).  The starved row keeps its INDEX and with it its place in the
 * blend order (main.cpp:419).  A rare, host-side call: it fetches statistics, parameters and moments, plans on the host,
 * writes the changed rows back the way s2d_rows_scatter does (projection and lists follow as they do there) and resets the
 * statistics.  *moved (may be NULL): pairs moved.  S2D_E_STATE without a statistics pass since the last reset;
 * S2D_E_INVALID for a slab context, a context with a held set (s2d_halo_commit) or S2D_CFG_REFERENCE_ORDER.  The
 * multi-device handle (s2d_multi) has no relocation: out of scope here. */
typedef struct s2d_relocate_config {
    uint32_t struct_size; /* = sizeof(s2d_relocate_config) */
    int32_t max_moves;    /* >= 0 */
    float min_weight;     /* per pass; +infinity: every splat counts as starved */
    float shrink;         /* 0 -> 1.6; otherwise > 0 */
} s2d_relocate_config;
int s2d_relocate(s2d_ctx* ctx, const s2d_relocate_config* cfg, int32_t* moved);

/* ---- importance-sampled placement (no counterpart in the reference, whose init() draws uniform positions and grey colours,
 * main.cpp:280-305).  Rows are drawn from a per-pixel importance map and written with the target's
 * colour there: a start that carries the picture (s2d_seed_splats over all rows), and a way to send unused splats to where
 * the picture is still wrong (s2d_reseed with S2D_SEED_ERROR).  Everything below is exact: two calls, or a NumPy restatement,
 * give the same bytes.  Pixels are numbered row-major, p = y * W + x; images are read as the context holds them (with
 * S2D_CFG_FP16_IMAGES: the fp16 values converted to fp32); all float arithmetic is fp32, one operation at a time.
 *
 * Importance q(p), a uint32, from a measure s in [0, 1]:
 *   S2D_SEED_TARGET_EDGES  y = imageRef; per channel e_c = |y_c(x+1,.) - y_c(x-1,.)| + |y_c(.,y+1) - y_c(.,y-1)|, indices
 *                          clamped to the image; m = (e_r + e_g) + e_b; s = min(1, m * 0.5f)
 *   S2D_SEED_ERROR         x = image0; d_c = |x_c - y_c|; m = (d_r + d_g) + d_b; s = min(1, m * (1.0f / 3.0f))
 *   S2D_SEED_CALLER        importance_device: H * W floats in DEVICE memory; s = the value clamped to [0, 1], NaN -> 0
 *   q0 = (uint32)(s * 4095.0f + 0.5f); with S2D_SEED_SQUARED q0 = (q0 * q0) >> 12; q = q0 + floor, floor in [0, 4095] being the
 *   uniform share; total = sum of q in 64 bits.
 * Draw of row i under `seed`, pcg3d as in init() (main.cpp:285-292), words mod 2^32:
 *   (ax, ay, az) = pcg3d(i, 2 * seed, 0x5EED5EED), (bx, by, bz) = pcg3d(i, 2 * seed + 1, 0x5EED5EED);
 *   u = floor(((ax * 2^32 + ay) * total) / 2^64); the pixel is the smallest p whose inclusive prefix sum of q exceeds u.
 * The row: pos = (clamp((float)x + (float)bx / 2^32, 0, W - 1), clamp((float)y + (float)by / 2^32, 0, H - 1)) -- the rasteriser's
 * pixel centre is x + 0.5; sx = sy = clamp(scale, 1, 1024), scale == 0 meaning sqrtf((float)W * (float)H / (float)n_splats);
 * rot = pi * ((float)az / 2^32); color = imageRef's rgb at the pixel clamped to [0, 1]; opacity as given, 0 meaning 1; all 18
 * Adam moments +0.  The draw depends on (i, seed) only: seeding a subset of rows writes exactly those rows of seeding all.
 *
 * S2D_E_INVALID, before any device work: a NULL config or wrong struct_size; an unknown source or flag; floor > 4095; a
 * negative or non-finite scale; opacity outside {0} and (0, 1]; S2D_SEED_CALLER with a NULL importance_device, another source
 * with a non-NULL one; ids out of range or repeated; a slab context (row_begin / row_end) or one with a held set
 * (s2d_halo_commit).  S2D_E_STATE: no target; S2D_SEED_ERROR without s2d_forward on the current parameters.  The multi-device
 * handle (s2d_multi) has no placement: out of scope here. */
#define S2D_SEED_TARGET_EDGES 0u
#define S2D_SEED_ERROR 1u
#define S2D_SEED_CALLER 2u
#define S2D_SEED_SQUARED 0x1u /* s2d_seed_config.flags */
typedef struct s2d_seed_config {
    uint32_t struct_size; /* = sizeof(s2d_seed_config) */
    uint32_t source;      /* S2D_SEED_TARGET_EDGES, _ERROR, _CALLER */
    uint32_t flags;       /* S2D_SEED_SQUARED */
    uint32_t seed;
    uint32_t floor;       /* 0 .. 4095 */
    float scale;          /* 0 -> sqrt(W * H / n_splats); otherwise finite and > 0, clamped to [1, 1024] */
    float opacity;        /* 0 -> 1; otherwise in (0, 1] */
    const float* importance_device; /* S2D_SEED_CALLER only */
} s2d_seed_config;
/* The map alone: q of every pixel (q_host: H * W words, may be NULL) and its total (may be NULL).  scale, opacity and seed
 * are checked but not used. */
int s2d_importance(s2d_ctx* ctx, const s2d_seed_config* cfg, uint32_t* q_host, uint64_t* total);
/* Writes the rows ids_host[0 .. count) (distinct; NULL: rows 0 .. count - 1, count <= n_splats) and zeroes their moments;
 * projection and lists follow as after s2d_rows_scatter.  beta1t / beta2t / iterations, the gradient buffer and the density
 * statistics are untouched: a caller who wants a fresh run calls s2d_init_splats first.  *placed (may be NULL): rows
 * written -- count, or 0 when the map's total is 0 (nothing is written then). */
int s2d_seed_splats(s2d_ctx* ctx, const s2d_seed_config* cfg, const int32_t* ids_host, int32_t count, int32_t* placed);
/* s2d_seed_splats over the STARVED rows of the density statistics: weight / passes < min_weight, ordered by (weight, index),
 * the first max_moves (rules 1-2 of csrc/s2d_density.h; no donors are involved).  Resets the statistics.  *moved (may be
 * NULL): rows written.  Additionally S2D_E_INVALID wherever s2d_relocate refuses (max_moves < 0, a NaN min_weight,
 * S2D_CFG_REFERENCE_ORDER) and S2D_E_STATE without a statistics pass since the last reset. */
int s2d_reseed(s2d_ctx* ctx, const s2d_seed_config* cfg, int32_t max_moves, float min_weight, int32_t* moved);

/* ---- image losses formed by the library (no counterpart in the reference, whose only loss is the squared error of
 * main.cpp:616).  With x = image0, y = imageRef, d = x - y, over all pixels p and channels c of .rgb:
 *
 *   L = sum_{p,c} [ w_mse * 1/2 * d^2  +  w_l1 * |d|  +  w_dssim * (1 - s) ]
 *
 * s is the SSIM index under the 11 x 11 Gaussian window w = g (x) g, g[i] = exp(-(i-5)^2 / (2 * 1.5^2)) normalised to sum 1,
 * with ZERO PADDING of 5 (pixels outside the image count as 0, the window is not renormalised: conv2d(padding=5)):
 *   mu_x = w*x, mu_y = w*y, var_x = w*x^2 - mu_x^2, var_y = w*y^2 - mu_y^2, cov = w*xy - mu_x mu_y, C1 = 0.01^2, C2 = 0.03^2,
 *   s = (2 mu_x mu_y + C1)(2 cov + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x + var_y + C2)).
 * L is a SUM, on the scale of the reference's gradient: dL/dx = w_mse * d + w_l1 * sign(d) + w_dssim * d(sum(1 - s))/dx with
 * sign(0) = 0, and weights (1, 0, 0) give image0 - imageRef, main.cpp:616, bit for bit.  The usual mix of means
 * (1 - lambda) * L1 + lambda * (1 - SSIM) is w_l1 = 1 - lambda, w_dssim = lambda up to the common factor 1 / (3 H W), which Adam's
 * normalisation removes.  A term whose weight is 0 is neither evaluated nor added; no window kernel runs when w_dssim == 0.
 * All arithmetic is fp32 on either image format; the sums are doubles added in a fixed order (no atomics: two calls give the
 * same bytes).
 * S2D_E_INVALID, before any device work: a NULL config or wrong struct_size; a negative or non-finite weight, or all three
 * zero; a slab context (row_begin / row_end) or one with a held set (s2d_halo_commit) -- the window crosses slab rows;
 * S2D_CFG_COUNT_PAIRS; S2D_BWD_DENSITY_STATS / S2D_STEP_DENSITY_STATS where s2d_backward refuses them.  S2D_E_STATE without
 * s2d_forward on the current parameters.  The multi-device handle (s2d_multi) has no loss but the squared error: out of
 * scope here. */
typedef struct s2d_loss_config {
    uint32_t struct_size; /* = sizeof(s2d_loss_config) */
    float w_mse, w_l1, w_dssim; /* each >= 0 and finite, not all 0 */
} s2d_loss_config;
/* MEANS over 3 * H * W of d^2, |d| and 1 - s, and total = w_mse * 1/2 * mse + w_l1 * l1 + w_dssim * dssim = L / (3 H W).  mse is on
 * the scale of the images ([0,1] channels): 255^2 * mse is what s2d_get_mse returns.  A term with weight 0 was not formed and
 * is NaN -- except mse, which every loss pass forms. */
typedef struct s2d_loss_terms {
    double mse, l1, dssim, total;
} s2d_loss_terms;
/* dL/d(image0) alone, into the caller's DEVICE buffer (height * width RGBA32F, .w = 0, 16-byte aligned), queued on the
 * context's stream; its terms are what s2d_loss_get returns next.  Touches neither the gradients nor the squared-error ring. */
int s2d_loss_image_grads_device(s2d_ctx* ctx, const s2d_loss_config* cfg, float* dimage_rows_device);
/* s2d_backward for the loss L: dL/d(image0) into an image the context owns (allocated by the first call, like the 9 floats
 * per pixel of scratch the window passes need), then the backward walk of s2d_backward_image_grads from it.  The squared
 * error of the iteration goes into the ring as after s2d_backward: s2d_get_mse and s2d_get_sqerr_trace keep working.
 * flags: S2D_BWD_SKIP_OPACITY_GRAD, S2D_BWD_DENSITY_STATS. */
int s2d_loss_backward(s2d_ctx* ctx, const s2d_loss_config* cfg, uint32_t flags);
/* The terms of the last loss pass (s2d_loss_backward, s2d_step_loss's last iteration or s2d_loss_image_grads_device);
 * S2D_E_STATE before any. */
int s2d_loss_get(s2d_ctx* ctx, s2d_loss_terms* out);
/* s2d_step with the loss L: per iteration s2d_forward, s2d_loss_backward, s2d_adam_step (image0 is stored every iteration).
 * loss_out (may be NULL): `total` of every iteration; mse_out (may be NULL): as for s2d_step.  flags:
 * S2D_STEP_OPTIMIZE_OPACITY, S2D_STEP_DENSITY_STATS.  S2D_E_NONFINITE and the NaN tail of both outputs as for s2d_step. */
int s2d_step_loss(s2d_ctx* ctx, int32_t iters, uint32_t flags, const s2d_loss_config* cfg, double* loss_out, double* mse_out);

/* Adam + constraints + finite guard, main.cpp:714-785, on the current gradient buffer; then iterations++ (809). */
int s2d_adam_step(s2d_ctx* ctx, uint32_t flags);

/* ---- optimiser controls (no counterpart in the reference, whose one trainingRate, main.cpp:715, drives all nine scalars of
 * a splat).  They act in the Adam launch, so s2d_adam_step, s2d_step (fused or with
 * S2D_STEP_DENSITY_STATS) and s2d_step_loss all follow them.
 *
 * Rates per parameter GROUP, with an optional log-linear decay.  The rate of group g for the step taken while the context's
 * `iterations` counter is t (the counter s2d_set_adam restores, so a resumed run continues its schedule):
 *   T == 0 or final_ratio[g] == 1 (0 means 1):  rate[g], exactly;
 *   otherwise:  (float)((double)rate[g] * pow((double)final_ratio[g], (double)min(t, T) / T)) -- constant from T on.
 * Every scalar of the group is then Adam::optimize (main.cpp:144-156) at that alpha, bit for bit.  The opacity rate matters
 * only under S2D_STEP_OPTIMIZE_OPACITY, as ever.
 *
 * FROZEN splats: the Adam step does not exist for them.  The 9 parameters, the 18 moments and the finite guard leave a frozen
 * splat alone (byte for byte); its gradient record is re-zeroed like everyone's (main.cpp:550).  The raster passes, the density
 * statistics, s2d_relocate and s2d_reseed do not know about the mask.  s2d_init_splats clears the mask (and keeps the rates);
 * s2d_set_splats, s2d_set_adam and the row calls keep both.  Setting either invalidates nothing.
 *
 * While a configuration or a mask is set -- even one that equals the defaults -- the step runs a second instantiation of the
 * Adam kernel; s2d_set_optim(NULL) with no mask returns to the plain one.
 * S2D_E_INVALID, before any device work, for all four calls: a slab context (row_begin / row_end) or one with a held set
 * (s2d_halo_commit; and s2d_halo_commit with masks refuses a context that has a configuration or a mask) -- the hold margins
 * of slab ownership are derived from the one training_rate; for s2d_set_optim also a wrong struct_size, a rate that is <= 0 or
 * not finite, a final_ratio that is negative or not finite, decay_iterations < 0; for s2d_optim_rates_at a negative iteration.
 * The multi-device handle (s2d_multi) has no such controls: out of scope here. */
/* groups: 0 pos (pos.x, pos.y), 1 scale (sx, sy), 2 rot, 3 colour (r, g, b), 4 opacity */
typedef struct s2d_optim_config {
    uint32_t struct_size;     /* = sizeof(s2d_optim_config) */
    float rate[5];            /* each finite and > 0 */
    float final_ratio[5];     /* 0 -> 1 (no decay); otherwise finite and > 0 */
    int32_t decay_iterations; /* T >= 0; 0 -> no decay, the ratios are not looked at beyond validation */
} s2d_optim_config;
int s2d_set_optim(s2d_ctx* ctx, const s2d_optim_config* cfg);        /* NULL: back to the single training_rate */
/* What the step taken at `iterations == iteration` uses (without a configuration: training_rate five times). */
int s2d_optim_rates_at(s2d_ctx* ctx, int32_t iteration, float rates[5]);
int s2d_set_frozen(s2d_ctx* ctx, const uint8_t* frozen_host);        /* n_splats bytes, non-zero = frozen; NULL: none */
int s2d_set_frozen_device(s2d_ctx* ctx, const uint8_t* frozen_device); /* copied on the context's stream; NULL: none */

/* ---- the alive set: how many splats take part (no counterpart in the reference, whose NSplat is fixed at init(),
 * main.cpp:271).  n_splats of s2d_config is the CAPACITY; a context may keep any subset of its rows
 * alive.  A dead row does not exist for the passes:
 *   raster      no footprint: empty tile rectangle, no list entry, no colour contribution; its gradient record stays +0;
 *   Adam        the step skips it: 9 parameters, 18 moments and the dormant byte stay byte for byte, the finite guard does
 *               not see it;
 *   statistics  its density statistics stay as they were (0 after a reset);
 *   blend order the row keeps its INDEX, which is its place in the blend order (main.cpp:419): a row that comes alive again
 *               is blended where its index says.
 * A context with an alive set draws exactly the image of a context that holds only the alive rows, in index order.
 * s2d_init_splats clears the set, as it clears the frozen mask; s2d_set_splats[_device], s2d_set_adam, the row calls,
 * s2d_set_optim and s2d_set_frozen keep it.  ANY change of the set -- departures too: a row that died would still cover its
 * pixels through its old list entries -- invalidates the tile lists, and the projection with them, before the next raster pass.
 * Everything works on a context with a set: s2d_forward, s2d_backward, s2d_forward_backward, s2d_step (fused and with
 * S2D_STEP_DENSITY_STATS), s2d_adam_step, s2d_backward_image_grads, the loss entry points, s2d_set_optim / s2d_set_frozen (a
 * row trains only when it is alive and not frozen), s2d_importance and s2d_seed_splats (seeding writes rows and does not
 * change which are alive), s2d_relocate and s2d_reseed (dead rows are neither starved nor donors), index-range rendering,
 * fp16 images, generic binning, counting and exact-exp contexts.
 * S2D_E_INVALID, before any device work, for the five calls below on a slab context (row_begin / row_end), a context with a
 * held set from s2d_halo_commit, or a S2D_CFG_REFERENCE_ORDER context; and s2d_halo_masks, and s2d_halo_commit with masks,
 * refuse a context that has an alive set.  The multi-device handle (s2d_multi) has no alive set: out of scope here. */
/* n_splats bytes, non-zero = alive; NULL: every row alive again (the buffers go). */
int s2d_set_alive(s2d_ctx* ctx, const uint8_t* alive_host);
int s2d_set_alive_device(s2d_ctx* ctx, const uint8_t* alive_device);   /* copied on the context's stream */
/* alive_host: n_splats bytes, each 0 or 1 (all 1 without a set); count: alive rows.  Either may be NULL. */
int s2d_get_alive(s2d_ctx* ctx, uint8_t* alive_host, int32_t* count);
/* alive' = alive AND NOT (criterion 1 OR criterion 2), decided on the device, one thread per row; a context without a set
 * starts from all ones.  *pruned (may be NULL): rows that died, from one read-back of the new count (one more, of the old
 * count, where the host does not know it: after s2d_set_alive_device).  With min_weight > 0 the
 * call needs a statistics pass since the last reset (S2D_E_STATE otherwise) and resets the statistics afterwards, as
 * s2d_relocate does.  No parameter or moment of any row is touched.  S2D_E_INVALID for a negative or NaN threshold, for both
 * thresholds 0, or for a wrong struct_size. */
typedef struct s2d_prune_config {
    uint32_t struct_size; /* = sizeof(s2d_prune_config) */
    float min_weight;     /* > 0: prune alive rows with (double)weight / (double)passes < (double)min_weight; 0: criterion off */
    float min_opacity;    /* > 0: prune alive rows with opacity < min_opacity; 0: off */
} s2d_prune_config;
int s2d_prune(s2d_ctx* ctx, const s2d_prune_config* cfg, int32_t* pruned);
/* Brings dead rows to life and seeds them.  ids_host: the rows -- distinct, in range, each currently dead, else
 * S2D_E_INVALID; NULL: the min(count, dead) dead rows of LOWEST index, the front-most free places in the blend order (so
 * that what is grown is not buried under what is there), chosen on the device from a scan over the dead flags.  The chosen
 * rows are written exactly as s2d_seed_splats writes those ids under the same config (same map, same draw per (i, seed),
 * moments +0; scale == 0 still means sqrt(W * H / n_splats) with n_splats the capacity), and all refusals and state rules of
 * s2d_seed_splats apply.  Then the rows are alive and the lists invalid; statistics, frozen mask and iteration counters are
 * untouched.  *grown (may be NULL): rows written -- 0 when the map's total is 0 (nothing changes then); no dead row, or
 * count == 0, gives S2D_OK with 0. */
int s2d_grow(s2d_ctx* ctx, const s2d_seed_config* cfg, const int32_t* ids_host, int32_t count, int32_t* grown);

/* ---- view rendering: the current splats at any zoom, crop and output size (no counterpart in the reference, which draws
 * image0 at the target's size only, main.cpp:414-546).  A VIEW is an axis-aligned window of the source
 * plane, drawn at a uniform zoom into a buffer of the caller's own size, with optional supersampling, an optional low-pass on
 * the footprints, and float or 8-bit output.  It is read-only with respect to training: image0, the tile lists and their
 * rebuild counters, the projection, the forward -> backward hand-over, the status word, the squared-error ring and the density
 * statistics are not touched, and a context trains on after a view -- or after a refused one -- as if nothing had been asked.
 *
 * The records a view rasterises, all arithmetic fp32, one operation at a time, s = samples (0 meaning 1):
 *   zr = zoom * (float)s;  fr = filter_var * (float)(s * s);
 *   pos' = ((pos.x - origin_x) * zr, (pos.y - origin_y) * zr);  ax = sx * zr;  ay = sy * zr;
 *   fr == 0:   sx' = ax, sy' = ay, opacity' = opacity;
 *   otherwise: sx' = sqrtf(ax * ax + fr), sy' = sqrtf(ay * ay + fr), opacity' = opacity * ((ax * ay) / (sx' * sy'));
 *   rot and colour unchanged.  Nothing is clamped.
 * They are rasterised by the reference's forward loop (main.cpp:414-546), in index order, the dead rows of an alive set left
 * out, on a grid of (out_width * s) x (out_height * s); S2D_CFG_EXACT_EXP is honoured, S2D_CFG_FP16_IMAGES and
 * S2D_CFG_COUNT_PAIRS play no part (a view is computed in fp32 and counts nothing).  The identity view (origin 0, zoom 1,
 * out = width x height, no filter, one sample) is image0 of s2d_forward byte for byte.
 * Resolve: s = 2: the output pixel is ((p00 + p01) + (p10 + p11)) * 0.25f per channel, p_rc at row r, column c of its 2 x 2
 * block of the grid; s = 4: that resolve applied twice; .w = 1.  No supersampled image exists in memory.
 * S2D_VIEW_RGBA8: per channel (uint8)(min(max(c, 0), 1) * 255.0f + 0.5f), NaN -> 0; alpha 255.
 * filter_var is defined exactly; nothing is claimed about the picture it gives.
 *
 * S2D_E_INVALID, before any device work: a NULL config or output; a wrong struct_size; sizes, zoom, origin, filter_var,
 * samples or format outside the ranges below; a device buffer that is not 16-byte (RGBA32F) or 4-byte (RGBA8) aligned; a slab
 * context (row_begin / row_end) or one with a held set (s2d_halo_commit).  S2D_E_NOMEM: the view's (tile, splat) pairs exceed
 * S2D_CHUNK_PAIRS (views are not rendered by index ranges), or an allocation failed.  There is no S2D_E_STATE: a view needs
 * splats, not a target or a forward pass.  The multi-device handle (s2d_multi) has no views: out of scope here. */
#define S2D_VIEW_RGBA32F 0u   /* out: out_height * out_width * 4 floats, .w = 1 (S2D_CFG_COVERAGE: coverage, resolved like the colours) */
#define S2D_VIEW_RGBA8   1u   /* out: out_height * out_width * 4 bytes,  .w = 255 (S2D_CFG_COVERAGE: coverage, quantised like the colours) */
typedef struct s2d_view_config {
    uint32_t struct_size;            /* = sizeof(s2d_view_config) */
    int32_t  out_width, out_height;  /* >= 1; out_* * samples <= 65536 */
    float    origin_x, origin_y;     /* source coordinates of the output's top-left corner; pixel i covers [i, i+1) */
    float    zoom;                   /* output pixels per source pixel; finite, > 0 */
    float    filter_var;             /* >= 0, finite: variance in OUTPUT pixels^2 of an isotropic low-pass; 0 = none */
    int32_t  samples;                /* per axis: 0 -> 1; 1, 2 or 4 */
    uint32_t format;                 /* S2D_VIEW_RGBA32F, S2D_VIEW_RGBA8 */
} s2d_view_config;
/* The n_splats records the view rasterises (dead rows are transformed like live ones). */
int s2d_view_splats(s2d_ctx* ctx, const s2d_view_config* cfg, s2d_splat* out_host);
/* The view into host memory; complete on return. */
int s2d_render_view(s2d_ctx* ctx, const s2d_view_config* cfg, void* out_host);
/* The view into DEVICE memory, queued on the context's stream (the host waits once, for the pair count of the list build). */
int s2d_render_view_device(s2d_ctx* ctx, const s2d_view_config* cfg, void* out_device);
/* Views allocate on first use and keep what they allocated -- the records, a projection and tile lists of the raster grid
 * (re-created when the grid's size changes, grown with the pair count), the device image behind s2d_render_view -- until this
 * call or s2d_destroy; the next view allocates again. */
int s2d_view_release(s2d_ctx* ctx);

/* ---- view gradients: the backward pass through a view, for coarse-to-fine, crop and supersampled
 * training.  s2d_view_backward_device queues, on the context's stream, the view's transform, projection and list build (the
 * one host wait of a view: the pair count), then ONE kernel that walks every tile of the raster grid forward and backward
 * (the final sample colours stay in registers; with samples > 1 the upstream gradient of an output pixel reaches the samples
 * of its block through lane reads, times 0.25f per resolve level -- no supersampled image or gradient exists in memory), on a
 * deterministic context the gather over the view's slots, and the adjoint of the record transform, which ADDS the result into
 * the gradient buffer s2d_backward and s2d_backward_image_grads accumulate into (the bound one after s2d_bind_grads_device):
 * s2d_adam_step afterwards steps on it and re-zeroes it as always.
 *
 * dview_or_target_device: out_height * out_width RGBA32F in device memory, 16-byte aligned, .w ignored -- dL/d(view), or with
 * S2D_VIEW_BWD_FROM_TARGET a TARGET of the view's size: the kernel forms dL = resolved - target itself, one fp32 subtraction
 * per channel (the gradient of sum (view - target)^2 / 2, the reference's loss at the view's size), so a C caller trains
 * against a small target with no elementwise kernel of its own.  No squared error is formed either way.
 * flags: S2D_VIEW_BWD_FROM_TARGET, S2D_BWD_SKIP_OPACITY_GRAD; anything else is S2D_E_INVALID.
 *
 * The adjoint of the records above, g' the gradient of a view record, k = (ax * ay) / (sx' * sy'), fp32, one operation at a
 * time, left to right:
 *   g_pos = g'_pos * zr;  g_rot = g'_rot;  g_col = g'_col;
 *   fr == 0:   g_sx = g'_sx * zr;  g_sy = g'_sy * zr;  g_op = g'_op;
 *   otherwise: g_op = g'_op * k;  t = (g'_op * opacity) * k;
 *              g_sx = zr * (g'_sx * (ax / sx') + t * (fr / (ax * (sx' * sx'))));  g_sy alike with y.
 * The row of a dead splat is left as it is.
 *
 * Otherwise the call is as read-only as a view: image0, the training lists and their rebuild counters, the projection, the
 * context's forward -> backward hand-over (the view has one of its own), the status word, the squared-error ring and the density
 * statistics are untouched.  It needs splats, not a target or a prior s2d_forward.  S2D_CFG_EXACT_EXP and
 * S2D_CFG_DETERMINISTIC are honoured (deterministic: bitwise reproducible, the slots being those of the view's rectangles).
 *
 * S2D_E_INVALID, before any device work: everything a view is refused for; format != S2D_VIEW_RGBA32F; a NULL or misaligned
 * pointer; unknown flags; a context with S2D_CFG_COUNT_PAIRS or S2D_CFG_REFERENCE_ORDER.  S2D_E_NOMEM as for a view; on top of
 * a view's buffers the pass keeps n x 9 floats, 36 bytes per pair of the lists' capacity for its hand-over and, deterministic,
 * 13 more words per pair -- all freed by s2d_view_release.  After a refusal the context trains on unchanged. */
#define S2D_VIEW_BWD_FROM_TARGET 0x8u
int s2d_view_backward_device(s2d_ctx* ctx, const s2d_view_config* cfg, const float* dview_or_target_device, uint32_t flags);
/* The same pass stopped before the adjoint of the record transform: the n_splats x 9 gradients of the VIEW's records (those of
 * s2d_view_splats) into host memory, complete on return; the context's gradient buffer is not touched.  An inspection seam: it
 * lets the two kernels be judged separately. */
int s2d_view_grads(s2d_ctx* ctx, const s2d_view_config* cfg, const float* dview_or_target_device, uint32_t flags,
                   s2d_splat* dview_records_host);

/* `iters` whole iterations (main.cpp:414-809): forward, backward, Adam, MSE.  mse_out (may be NULL) receives
 * iters doubles: the value the reference prints for each iteration (main.cpp:796-807).  For a slab context the
 * values are this slab's sum of squared errors divided by (H*W*3), i.e. partial MSEs that add up over slabs.
 * Returns S2D_E_NONFINITE where the reference would abort(). */
int s2d_step(s2d_ctx* ctx, int32_t iters, uint32_t flags, double* mse_out);

/* MSE (main.cpp:796-805) of the framebuffer produced by the last s2d_forward / s2d_backward pair. */
int s2d_get_mse(s2d_ctx* ctx, double* mse);

/* ---- Slab ownership for multi-GPU runs (no counterpart in the reference, which is single-process; DESIGN.md
 * section 7, SURVEY.md section 8e "neighbour-only exchange").  A rank HOLDS splat i while the rows
 * [pos.y - reach - margin, pos.y + reach + margin], reach = 3*max(sx, sy) + 2 (the circle bounding the y-range of
 * main.cpp:489-491), meet its row slab.  Only held splats are projected, listed and updated by s2d_adam_step; the
 * host keeps the holders' copies identical by exchanging gradient rows (and, when a splat drifts into another
 * rank's halo, its 27-float state).  All pointers are DEVICE pointers owned by the caller; work is queued on the
 * context's stream. */
#define S2D_ROWS_GRADS 0  /* 9 floats per row: the gradient buffer (s2d_bind_grads_device or internal) */
#define S2D_ROWS_SPLATS 1 /* 9 floats per row: s2d_splat */
#define S2D_ROWS_ADAM 2   /* 18 floats per row: s2d_splat_adam */
/* masks[i] bit q = rank q holds splat i under the current parameters (row_bounds: world+1 host ints, rank q owns
 * rows row_bounds[q] .. row_bounds[q+1]); 0 for splats this context does not hold. world <= 32. */
int s2d_halo_masks(s2d_ctx* ctx, int32_t world, const int32_t* row_bounds, float margin_rows, uint32_t* masks_device);
/* This context holds exactly the splats with bit `rank` set.  added != 0: splats this context did not hold before
 * are among them (their rows were written with s2d_rows_scatter): the tile lists are rebuilt before the next
 * forward.  Splats that merely left keep their (now empty) list entries until the next regular rebuild.
 * masks_device == NULL: the context holds every splat again (its copy of all rows must be current). */
int s2d_halo_commit(s2d_ctx* ctx, const uint32_t* masks_device, int32_t rank, int32_t added);
/* out[j] = row ids[j] of the chosen array / row ids[j] = in[j] (ids distinct; out-of-range ids read 0 / are skipped) */
int s2d_rows_gather(s2d_ctx* ctx, int32_t what, const int32_t* ids_device, int32_t count, float* out_device);
int s2d_rows_scatter(s2d_ctx* ctx, int32_t what, const int32_t* ids_device, int32_t count, const float* in_device);
/* grads[rows[u]] = sum over ranks q = 0..world-1, in that order, of rank q's partial: src[u*world + q] = -1 (q does
 * not hold the row), -2 (q is this rank: the partial already in the gradient buffer), or a row index into recv.
 * The fixed order makes the sum bit-identical on every holder. */
int s2d_grads_combine(s2d_ctx* ctx, const int32_t* rows_device, int32_t n_rows, const int32_t* src_device, int32_t world,
                      const float* recv_device);

/* ---- multi-GPU plumbing (one process per GPU; the caller's collective runs between s2d_forward_backward and
 * s2d_adam_step, on the context's stream) ---- */
/* Use caller-owned DEVICE memory (n_splats * 9 floats, layout s2d_splat[n]) as the gradient buffer, so the host
 * can all-reduce it in place (RCCL).  NULL -> back to the context's own buffer.  The buffer must be 16-byte
 * aligned, zero when bound, and is re-zeroed by s2d_adam_step. */
int s2d_bind_grads_device(s2d_ctx* ctx, void* grads_device);
/* Device address of the gradient buffer currently in use. */
void* s2d_grads_device_ptr(s2d_ctx* ctx);
/* The hipStream_t the context queues its work on (s2d_config.stream, or the one it created): a caller that puts its
 * own device work between two calls -- the RCCL all-reduce and the peer copies of s2d_multi -- queues it here. */
void* s2d_stream(s2d_ctx* ctx);
/* Per-iteration sums of squared errors of this slab kept on the device (ring of `capacity` doubles indexed by
 * iteration % capacity); lets a multi-GPU host reduce them once after many steps instead of every iteration. */
int s2d_get_sqerr_trace(s2d_ctx* ctx, int32_t first_iteration, int32_t count, double* out);
int s2d_synchronize(s2d_ctx* ctx);

/* ---- several GPUs behind one handle ("device list ...; multi-GPU fan-out is internal") -------------
 * s2d_multi keeps the single-threaded call pattern of main.cpp:334 and runs it on n_devices GPUs: the image is cut into
 * n_devices row slabs (whole 16-pixel tile rows), every device gets an ordinary context for its slab and a worker thread
 * inside the library; the caller needs none.  cfg: as for s2d_create, with device / row_begin / row_end / stream unused
 * (must be 0).  Keeping the devices consistent:
 *  - default, slab ownership: a device holds and updates only the splats that can reach its rows; per iteration the
 *    holders of a shared splat swap its partial gradient rows by peer-to-peer copies (xGMI) and add them in rank order;
 *    every 64 iterations the hold sets follow the parameters and the state of a splat entering a neighbour's reach is
 *    handed over.  get_splats / get_adam assemble the arrays from the holders.
 *  - S2D_MULTI_REPLICATED (north_star's scheme): splats and Adam state on every device, the N x 9 fp32 gradient arrays
 *    summed in place by an RCCL all-reduce (on each context's stream, between s2d_forward_backward and s2d_adam_step),
 *    the identical Adam step everywhere.  RCCL is loaded (dlopen) when such a handle is created.
 * With deterministic gradients (S2D_CFG_DETERMINISTIC) and sums formed in rank order the two give the same bits.
 * After a failed s2d_multi_step (S2D_E_NONFINITE: the reference abort()s there; or one rank's own failure, reported with that
 * rank's number and message) the ranks stand at different iterations and the state is for inspection only: further steps are
 * refused (S2D_E_STATE) until s2d_multi_init_splats, or s2d_multi_set_splats + s2d_multi_set_adam, set it afresh -- unless a
 * collective had to be aborted or a rank stopped answering (s2d_multi_set_stall_timeout): then the handle must be re-created. */
#define S2D_MULTI_SHARE_GPU 0x1u  /* rehearsal on a box with fewer GPUs than ranks: all ranks on devices[0]; peer copies
                                   * become device copies, the all-reduce is staged through pinned host memory in rank
                                   * order (RCCL takes one rank per GPU) */
#define S2D_MULTI_REPLICATED 0x2u /* replicated state + all-reduce of all gradients instead of slab ownership */
typedef struct s2d_multi s2d_multi;
int s2d_multi_create(const s2d_config* cfg, const int32_t* devices, int32_t n_devices, uint32_t flags, s2d_multi** out);
void s2d_multi_destroy(s2d_multi* m);
const char* s2d_multi_last_error(const s2d_multi* m);
int s2d_multi_device_count(const s2d_multi* m);
/* Which GPU runs which rows: HIP device ordinal, row slab [row_begin, row_end), PCI bus id ("0000:c1:00.0") and marketing
 * name of rank `rank`'s device (any output may be NULL; strings are truncated to their capacity).  What a host prints so
 * that a multi-GPU record proves N distinct devices took part. */
int s2d_multi_device_info(s2d_multi* m, int32_t rank, int32_t* device, int32_t* row_begin, int32_t* row_end, char* pci_bus_id,
                          int32_t pci_capacity, char* name, int32_t name_capacity);
/* A rank that stops answering must not hang the caller (the reference's only failure policy is abort(), main.cpp:752-785;
 * this boundary turns failures into statuses, and "a rank stopped answering" is one of them).  Every wait of one rank for
 * another -- for the event of its gradient exchange, at the rendezvous of a hold-set refresh -- and for its own stream
 * gives up after `milliseconds` without progress: the step returns S2D_E_STATE, s2d_multi_last_error names the rank, the
 * exchange / iteration and what it was last seen doing, communicators are aborted, and the handle refuses further work
 * until it is destroyed and created again.  A rank that does not even answer the stop (it sits inside a runtime call) is
 * abandoned after about three times the limit: the call still returns.  Default 30 000 (S2D_MULTI_STALL_TIMEOUT_MS in the
 * environment overrides it at creation); 0 = wait without bound. */
int s2d_multi_set_stall_timeout(s2d_multi* m, int32_t milliseconds);
int s2d_multi_set_target(s2d_multi* m, const float* rgba32f);         /* imageRef, main.cpp:254-259, to every replica */
int s2d_multi_set_target_synthetic(s2d_multi* m);
int s2d_multi_init_splats(s2d_multi* m);                              /* init(), main.cpp:280-305, on every replica */
int s2d_multi_set_splats(s2d_multi* m, const s2d_splat* splats);
int s2d_multi_get_splats(s2d_multi* m, s2d_splat* splats);            /* every row from its lowest-ranked holder */
int s2d_multi_set_adam(s2d_multi* m, const s2d_splat_adam* adams, float beta1t, float beta2t, int32_t iterations);
int s2d_multi_get_adam(s2d_multi* m, s2d_splat_adam* adams, float* beta1t, float* beta2t, int32_t* iterations);
/* `iters` whole iterations (main.cpp:414-809) on all devices; mse_out as for s2d_step (the slabs' squared errors are
 * added in slab order).  S2D_E_NONFINITE where the reference would abort(). */
int s2d_multi_step(s2d_multi* m, int32_t iters, uint32_t flags, double* mse_out);
/* Forward rasteriser (main.cpp:414-546) of the current parameters on every device's rows, e.g. for display (main.cpp:794). */
int s2d_multi_forward(s2d_multi* m);
/* image0 of the last s2d_multi_forward, or of the last iteration of the last s2d_multi_step, assembled from the slabs. */
int s2d_multi_get_image(s2d_multi* m, float* rgba32f);
/* out4: scheme in use (0 none: one device, 1 slab ownership, 2 replicated), gradient rows swapped per iteration (all
 * ranks), state rows handed over so far, splats held summed over the ranks (n_splats * n_devices when replicated). */
int s2d_multi_exchange_info(s2d_multi* m, int64_t* out4);

/* out->struct_size must be set by the caller (S2D_E_INVALID when it is smaller than the first version of the struct). */
int s2d_get_stats(s2d_ctx* ctx, s2d_stats* out);
/* s2d_stats.rebins without the device round trip s2d_get_stats makes (a host-side counter; never synchronises). */
int s2d_get_rebuild_count(const s2d_ctx* ctx, uint64_t* rebuilds);
const char* s2d_last_error(const s2d_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* SPLAT2D_H */
