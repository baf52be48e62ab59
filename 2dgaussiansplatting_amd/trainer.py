"""Trainer: one context of the library (s2d_ctx) -- the reference's training state and its three passes on one MI355X."""
import contextlib
import ctypes as C
import os

import numpy as np

from ._abi import (S2D_BWD_DENSITY_STATS, S2D_BWD_SKIP_OPACITY_GRAD, S2D_CFG_ADAM_FP32, S2D_CFG_COUNT_PAIRS,
                   S2D_CFG_COVERAGE, S2D_CFG_DETERMINISTIC, S2D_CFG_EXACT_EXP, S2D_CFG_FP16_IMAGES, S2D_CFG_GENERIC_BINNING,
                   S2D_CFG_REFERENCE_ORDER, S2D_FB_SKIP_IMAGE, S2D_SEED_SQUARED, S2D_STEP_DENSITY_STATS,
                   S2D_STEP_OPTIMIZE_OPACITY, S2D_VIEW_BWD_FROM_TARGET, S2D_VIEW_RGBA8, S2D_VIEW_RGBA32F, SEED_SOURCES,
                   SPLAT_DTYPE, _Config, _LossConfig, _LossTerms, _OptimConfig, _PruneConfig, _RelocateConfig, _SeedConfig,
                   _Stats, _ViewConfig)
from ._handle import _Handle, _p


def _dev(ptr):
    """A device address (an integer; 0 or None: the call's "no buffer") as the void pointer argument."""
    return C.c_void_p(ptr) if ptr else None


@contextlib.contextmanager
def _chunk_pairs_env(chunk_pairs):
    """S2D_CHUNK_PAIRS is `chunk_pairs` inside the block and exactly what it was afterwards; None leaves it alone."""
    old = os.environ.get("S2D_CHUNK_PAIRS")
    if chunk_pairs is not None:
        os.environ["S2D_CHUNK_PAIRS"] = str(int(chunk_pairs))
    try:
        yield
    finally:
        if chunk_pairs is not None:
            if old is None:
                del os.environ["S2D_CHUNK_PAIRS"]
            else:
                os.environ["S2D_CHUNK_PAIRS"] = old


class Trainer(_Handle):
    """The reference's training state and its three passes, on one MI355X (or one row slab of the image).

    Mirrors main()'s locals: splats / splatAdams / beta1t / beta2t / iterations (main.cpp:272-278),
    imageRef (:254), image0 (:310), optimizeOpacity (:317).
    """

    _PREFIX = "s2d_"

    def __init__(self, width, height, n_splats, device=0, row_begin=0, row_end=0, training_rate=0.0,
                 rebin_interval=0, rebin_margin=0.0, count_pairs=False, fp16_images=False, deterministic=False, exact_exp=False,
                 adam_fp32=False, generic_binning=False, stream=None, chunk_pairs=None, reference_order=False, coverage=False):
        self.W, self.H, self.n = int(width), int(height), int(n_splats)
        cfg = _Config()
        cfg.struct_size = C.sizeof(_Config)
        cfg.width, cfg.height, cfg.n_splats, cfg.device = self.W, self.H, self.n, int(device)
        cfg.row_begin, cfg.row_end = int(row_begin), int(row_end)
        self.row_begin, self.row_end = (0, self.H) if (int(row_begin), int(row_end)) == (0, 0) else (int(row_begin), int(row_end))
        cfg.training_rate = float(training_rate)
        cfg.flags = ((S2D_CFG_COUNT_PAIRS if count_pairs else 0) | (S2D_CFG_FP16_IMAGES if fp16_images else 0) |
                     (S2D_CFG_DETERMINISTIC if deterministic else 0) | (S2D_CFG_EXACT_EXP if exact_exp else 0) |
                     (S2D_CFG_ADAM_FP32 if adam_fp32 else 0) | (S2D_CFG_GENERIC_BINNING if generic_binning else 0) |
                     (S2D_CFG_REFERENCE_ORDER if reference_order else 0) | (S2D_CFG_COVERAGE if coverage else 0))
        cfg.rebin_interval = int(rebin_interval)
        cfg.rebin_margin = float(rebin_margin)
        cfg.stream = stream
        self.stream = stream  # HIP stream handle the context works on; None: a stream the library owns
        # reference_order: validation mode, gradients / optimiser state / MSE bytes-equal to the reference's
        # (S2D_CFG_REFERENCE_ORDER, include/splat2d.h); slower and memory-hungry, results otherwise those of the reference
        # coverage: image0.w, the target's .w and the .w of a caller's image gradient are the coverage channel
        # (S2D_CFG_COVERAGE, include/splat2d.h) instead of a constant 1 / ignored
        # chunk_pairs (tests): the (tile, splat) pair budget beyond which a scene is rendered by index ranges of the splats;
        # the library reads S2D_CHUNK_PAIRS when the context is created (default 2^30)
        with _chunk_pairs_env(chunk_pairs):
            self._create(C.byref(cfg))
        self.training_rate = float(training_rate) if training_rate > 0 else 0.05  # main.cpp:715
        self.optimize_opacity = False  # main.cpp:317
        self.lean_backward = False     # backward() may skip the opacity gradient while optimize_opacity is off

    def _flags(self):
        return S2D_STEP_OPTIMIZE_OPACITY if self.optimize_opacity else 0

    def _bwd_flags(self, skip_opacity_grad, density_stats=False):
        """The flags of a backward pass.  skip_opacity_grad=None: skip dSplats.opacity exactly when optimize_opacity is off and
        `lean_backward` was requested (bench / training loops); False: always compute it, as the reference does."""
        if skip_opacity_grad is None:
            skip_opacity_grad = self.lean_backward and not self.optimize_opacity
        return (S2D_BWD_SKIP_OPACITY_GRAD if skip_opacity_grad else 0) | (S2D_BWD_DENSITY_STATS if density_stats else 0)

    # -- the three passes (set_target .. forward and get_image: _Handle)
    def get_image_rows(self):
        """The slab's rows of image0 only (row_begin .. row_end)."""
        a = np.zeros((self.row_end - self.row_begin, self.W, 4), dtype=np.float32)
        self._ck(self.L.s2d_get_image_rows(self._h, _p(a)))
        return a

    def backward(self, skip_opacity_grad=None, density_stats=False):
        """Backward pass.  skip_opacity_grad: see _bwd_flags.
        density_stats: the pass also accumulates the density statistics (S2D_BWD_DENSITY_STATS, density())."""
        self._ck(self.L.s2d_backward(self._h, self._bwd_flags(skip_opacity_grad, density_stats)))

    def forward_backward(self, skip_opacity_grad=None, skip_image=False):
        """forward() + backward() in one launch per tile (same results); skip_opacity_grad as backward();
        skip_image: do not store image0 (S2D_FB_SKIP_IMAGE)."""
        self._ck(self.L.s2d_forward_backward(self._h, self._bwd_flags(skip_opacity_grad) | (S2D_FB_SKIP_IMAGE if skip_image else 0)))

    def get_grads(self):
        a = np.zeros(self.n, dtype=SPLAT_DTYPE)
        self._ck(self.L.s2d_get_grads(self._h, _p(a)))
        return a

    # -- the rasteriser as a building block: raw DEVICE pointers, work queued on the context's stream, no host
    # synchronisation (torch_op.SplatRenderer wraps these around torch tensors)
    def set_splats_device(self, ptr):
        """The n x 9 float parameters from device memory (s2d_set_splats_device)."""
        self._ck(self.L.s2d_set_splats_device(self._h, _dev(ptr)))

    def get_image_rows_device(self, ptr):
        """The slab's rows of image0 into device memory, always RGBA32F (s2d_get_image_rows_device)."""
        self._ck(self.L.s2d_get_image_rows_device(self._h, _dev(ptr)))

    def backward_image_grads(self, ptr, skip_opacity_grad=None, density_stats=False):
        """Backward pass from the caller's dL/d(image0) (device pointer, the slab's rows, RGBA32F, .w ignored -- a coverage context:
        .w = dL/d(coverage)) instead of
        image0 - imageRef; skip_opacity_grad and density_stats as backward()."""
        self._ck(self.L.s2d_backward_image_grads(self._h, _dev(ptr), self._bwd_flags(skip_opacity_grad, density_stats)))

    def adam_step(self):
        self._ck(self.L.s2d_adam_step(self._h, self._flags()))

    def step(self, iters=1, want_mse=True, density_stats=False):
        """iters whole iterations; returns the MSE values the reference would print (main.cpp:807).  density_stats: every
        iteration is a statistics pass (S2D_STEP_DENSITY_STATS: the separate launches instead of the fused one)."""
        out = np.zeros(iters, dtype=np.float64) if want_mse else None
        flags = self._flags() | (S2D_STEP_DENSITY_STATS if density_stats else 0)
        self._ck(self.L.s2d_step(self._h, int(iters), flags, _p(out) if want_mse else None))
        return out

    # -- image losses formed by the library (include/splat2d.h, "image losses"): L = sum of w_mse * d^2 / 2 + w_l1 * |d| +
    # w_dssim * (1 - SSIM) over pixels and channels; a term with weight 0 is not evaluated
    @staticmethod
    def _loss_config(w_mse, w_l1, w_dssim):
        return _LossConfig(C.sizeof(_LossConfig), float(w_mse), float(w_l1), float(w_dssim))

    def loss_image_grads_device(self, ptr, w_mse, w_l1, w_dssim):
        """dL/d(image0) of the current frame alone into device memory (H x W RGBA32F, .w = 0, 16-byte aligned), queued on
        the context's stream; loss_terms() then returns this pass's terms."""
        cfg = self._loss_config(w_mse, w_l1, w_dssim)
        self._ck(self.L.s2d_loss_image_grads_device(self._h, C.byref(cfg), _dev(ptr)))

    def loss_backward(self, w_mse, w_l1, w_dssim, skip_opacity_grad=None, density_stats=False):
        """backward() for the loss L (s2d_loss_backward); skip_opacity_grad and density_stats as backward()."""
        cfg = self._loss_config(w_mse, w_l1, w_dssim)
        self._ck(self.L.s2d_loss_backward(self._h, C.byref(cfg), self._bwd_flags(skip_opacity_grad, density_stats)))

    def loss_terms(self):
        """-> dict(mse, l1, dssim, total) of the last loss pass: means over 3 * H * W, NaN for a term whose weight was 0
        (mse is always formed; 255^2 * mse is what mse() returns)."""
        t = _LossTerms()
        self._ck(self.L.s2d_loss_get(self._h, C.byref(t)))
        return {"mse": t.mse, "l1": t.l1, "dssim": t.dssim, "total": t.total}

    def step_loss(self, iters, w_mse, w_l1, w_dssim, want=True, density_stats=False):
        """iters whole iterations with the loss L (s2d_step_loss); returns (loss, mse): `total` of every iteration and the
        MSE values of step(), or (None, None) with want=False."""
        loss = np.zeros(iters, dtype=np.float64) if want else None
        mse = np.zeros(iters, dtype=np.float64) if want else None
        cfg = self._loss_config(w_mse, w_l1, w_dssim)
        flags = self._flags() | (S2D_STEP_DENSITY_STATS if density_stats else 0)
        self._ck(self.L.s2d_step_loss(self._h, int(iters), flags, C.byref(cfg), _p(loss) if want else None,
                                      _p(mse) if want else None))
        return loss, mse

    # -- optimiser controls (include/splat2d.h, "optimiser controls"): they act in the Adam launch of adam_step(), step() and
    # step_loss() alike
    _UNSET = object()

    def set_optim(self, pos=_UNSET, scale=None, rot=None, color=None, opacity=None, final_ratio=None, decay_iterations=0):
        """s2d_set_optim: a rate per parameter group (an omitted one: the context's training_rate), optionally decaying
        log-linearly to rate * final_ratio[g] over decay_iterations (final_ratio: five numbers in the order pos, scale, rot,
        color, opacity, 0 or 1 meaning no decay; or one number for all).  set_optim(None): back to the single training_rate."""
        if pos is None:
            self._ck(self.L.s2d_set_optim(self._h, None))
            return
        cfg = _OptimConfig()
        cfg.struct_size = C.sizeof(_OptimConfig)
        for g, r in enumerate((None if pos is Trainer._UNSET else pos, scale, rot, color, opacity)):
            cfg.rate[g] = self.training_rate if r is None else float(r)
        if final_ratio is not None:
            ratios = [float(final_ratio)] * 5 if np.isscalar(final_ratio) else [float(x) for x in final_ratio]
            assert len(ratios) == 5, ratios
            for g in range(5):
                cfg.final_ratio[g] = ratios[g]
        cfg.decay_iterations = int(decay_iterations)
        self._ck(self.L.s2d_set_optim(self._h, C.byref(cfg)))

    def rates_at(self, iteration):
        """-> five float32: the rates (pos, scale, rot, color, opacity) of the step taken while `iterations == iteration`."""
        out = np.zeros(5, dtype=np.float32)
        self._ck(self.L.s2d_optim_rates_at(self._h, int(iteration), _p(out)))
        return out

    def set_frozen(self, mask):
        """s2d_set_frozen: n booleans / bytes, non-zero = the Adam step does not exist for that splat; None: no mask."""
        if mask is None:
            self._ck(self.L.s2d_set_frozen(self._h, None))
            return
        a = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert a.shape == (self.n,), a.shape
        self._ck(self.L.s2d_set_frozen(self._h, _p(a)))

    def set_frozen_device(self, ptr):
        """The same from n bytes of device memory, copied on the context's stream (0 / None: no mask)."""
        self._ck(self.L.s2d_set_frozen_device(self._h, _dev(ptr)))

    # -- the alive set (include/splat2d.h, "the alive set")
    def set_alive(self, mask):
        """s2d_set_alive: n booleans / bytes, non-zero = the row takes part; None: every row again.  A dead row is not drawn,
        listed or stepped and keeps its index (its place in the blend order)."""
        if mask is None:
            self._ck(self.L.s2d_set_alive(self._h, None))
            return
        a = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert a.shape == (self.n,), a.shape
        self._ck(self.L.s2d_set_alive(self._h, _p(a)))

    def set_alive_device(self, ptr):
        """The same from n bytes of device memory, copied on the context's stream (0 / None: every row again)."""
        self._ck(self.L.s2d_set_alive_device(self._h, _dev(ptr)))

    def alive(self):
        """-> (n booleans, the number of alive rows); all True without a set."""
        a = np.zeros(self.n, dtype=np.uint8)
        count = C.c_int32()
        self._ck(self.L.s2d_get_alive(self._h, _p(a), C.byref(count)))
        return a != 0, count.value

    def prune(self, min_weight=0.0, min_opacity=0.0):
        """s2d_prune: alive rows with weight per statistics pass < min_weight or opacity < min_opacity die (a threshold of 0
        is off); returns their number.  With min_weight the statistics are reset."""
        cfg = _PruneConfig(C.sizeof(_PruneConfig), float(min_weight), float(min_opacity))
        pruned = C.c_int32()
        self._ck(self.L.s2d_prune(self._h, C.byref(cfg), C.byref(pruned)))
        return pruned.value

    def grow(self, count, ids=None, source="edges", squared=False, floor=0, scale=0.0, opacity=0.0, seed=0, importance_ptr=None):
        """s2d_grow: the rows `ids` (each dead), or with None the `count` dead rows of lowest index, are seeded as seed()
        seeds them and come alive; returns the number of rows written (0 for an all-zero map or without a dead row)."""
        cfg = self._seed_config(source, squared, floor, scale, opacity, seed, importance_ptr)
        grown = C.c_int32()
        if ids is None:
            self._ck(self.L.s2d_grow(self._h, C.byref(cfg), None, min(int(count), 2**31 - 1), C.byref(grown)))
        else:
            a = np.ascontiguousarray(ids, dtype=np.int32)
            self._ck(self.L.s2d_grow(self._h, C.byref(cfg), _p(a), len(a), C.byref(grown)))
        return grown.value

    # -- density control (include/splat2d.h, "density control")
    def density(self):
        """-> ((n, 3) float32: sum |dpos.x|, sum |dpos.y|, sum T * alpha over the accumulated passes, and their number)."""
        a = np.zeros((self.n, 3), dtype=np.float32)
        passes = C.c_int32()
        self._ck(self.L.s2d_density_get(self._h, _p(a), C.byref(passes)))
        return a, passes.value

    def density_device(self, ptr):
        """The same n x 3 floats into device memory, queued on the context's stream; returns the number of passes."""
        passes = C.c_int32()
        self._ck(self.L.s2d_density_get_device(self._h, _dev(ptr), C.byref(passes)))
        return passes.value

    def density_reset(self):
        self._ck(self.L.s2d_density_reset(self._h))

    def relocate(self, max_moves, min_weight, shrink=0.0):
        """s2d_relocate: starved splats (weight per pass < min_weight) onto halves of the splats with the largest summed
        |dpos|; returns the number of pairs moved.  The statistics are reset."""
        cfg = _RelocateConfig(C.sizeof(_RelocateConfig), int(max_moves), float(min_weight), float(shrink))
        moved = C.c_int32()
        self._ck(self.L.s2d_relocate(self._h, C.byref(cfg), C.byref(moved)))
        return moved.value

    # -- importance-sampled placement (include/splat2d.h, "importance-sampled placement")
    @staticmethod
    def _seed_config(source, squared, floor, scale, opacity, seed, importance_ptr):
        src = SEED_SOURCES[source] if isinstance(source, str) else int(source)
        return _SeedConfig(C.sizeof(_SeedConfig), src, S2D_SEED_SQUARED if squared else 0, int(seed) & 0xFFFFFFFF, int(floor),
                           float(scale), float(opacity), _dev(importance_ptr))

    def importance(self, source="edges", squared=False, floor=0, importance_ptr=None):
        """The importance map of the current images: -> ((H, W) uint32 q, total).  source: "edges" (the target's central
        differences), "error" (|image0 - target|, needs forward()) or "caller" (importance_ptr: H * W floats in device memory)."""
        cfg = self._seed_config(source, squared, floor, 0.0, 0.0, 0, importance_ptr)
        q = np.zeros((self.H, self.W), dtype=np.uint32)
        total = C.c_uint64()
        self._ck(self.L.s2d_importance(self._h, C.byref(cfg), _p(q), C.byref(total)))
        return q, total.value

    def seed(self, ids=None, source="edges", squared=False, floor=0, scale=0.0, opacity=0.0, seed=0, importance_ptr=None,
             count=None):
        """s2d_seed_splats: the rows `ids` (None: rows 0 .. count - 1, count None: all) drawn from the importance map and
        written with the target's colour, moments zeroed; returns the number of rows written (0 for an all-zero map)."""
        cfg = self._seed_config(source, squared, floor, scale, opacity, seed, importance_ptr)
        placed = C.c_int32()
        if ids is None:
            self._ck(self.L.s2d_seed_splats(self._h, C.byref(cfg), None, self.n if count is None else int(count), C.byref(placed)))
        else:
            a = np.ascontiguousarray(ids, dtype=np.int32)
            self._ck(self.L.s2d_seed_splats(self._h, C.byref(cfg), _p(a), len(a), C.byref(placed)))
        return placed.value

    def reseed(self, max_moves, min_weight, source="error", squared=False, floor=0, scale=0.0, opacity=0.0, seed=0,
               importance_ptr=None):
        """s2d_reseed: seed() over the starved rows of the density statistics (weight per pass < min_weight, the lowest
        first, at most max_moves); returns the number of rows written.  The statistics are reset."""
        cfg = self._seed_config(source, squared, floor, scale, opacity, seed, importance_ptr)
        moved = C.c_int32()
        self._ck(self.L.s2d_reseed(self._h, C.byref(cfg), int(max_moves), float(min_weight), C.byref(moved)))
        return moved.value

    # -- view rendering (s2d_view_config, include/splat2d.h): the current splats at any zoom, crop and output size; read-only
    # with respect to training
    @staticmethod
    def _view_config(out_width, out_height, origin=(0.0, 0.0), zoom=1.0, filter_var=0.0, samples=1, rgba8=False):
        cfg = _ViewConfig()
        cfg.struct_size = C.sizeof(_ViewConfig)
        cfg.out_width, cfg.out_height = int(out_width), int(out_height)
        cfg.origin_x, cfg.origin_y = float(origin[0]), float(origin[1])
        cfg.zoom, cfg.filter_var, cfg.samples = float(zoom), float(filter_var), int(samples)
        cfg.format = S2D_VIEW_RGBA8 if rgba8 else S2D_VIEW_RGBA32F
        return cfg

    def view_splats(self, out_width, out_height, origin=(0.0, 0.0), zoom=1.0, filter_var=0.0, samples=1, rgba8=False):
        """The n records the view rasterises (the transform of include/splat2d.h; dead rows like live ones)."""
        cfg = self._view_config(out_width, out_height, origin, zoom, filter_var, samples, rgba8)
        a = np.zeros(self.n, dtype=SPLAT_DTYPE)
        self._ck(self.L.s2d_view_splats(self._h, C.byref(cfg), _p(a)))
        return a

    def render_view(self, out_width, out_height, origin=(0.0, 0.0), zoom=1.0, filter_var=0.0, samples=1, rgba8=False):
        """The window of the source plane that starts at `origin`, at `zoom` output pixels per source pixel, as an
        (out_height, out_width, 4) array: float32 with .w = 1, or uint8 with alpha 255 (rgba8); a coverage context: .w = coverage.  samples: 1, 2 or 4 per axis;
        filter_var: variance, in output pixels^2, of a low-pass on the footprints."""
        cfg = self._view_config(out_width, out_height, origin, zoom, filter_var, samples, rgba8)
        a = np.zeros((int(out_height), int(out_width), 4), dtype=np.uint8 if rgba8 else np.float32)
        self._ck(self.L.s2d_render_view(self._h, C.byref(cfg), _p(a)))
        return a

    def render_view_device(self, ptr, out_width, out_height, origin=(0.0, 0.0), zoom=1.0, filter_var=0.0, samples=1, rgba8=False):
        """render_view into device memory (16-byte aligned for float32, 4-byte for rgba8), queued on the context's stream."""
        cfg = self._view_config(out_width, out_height, origin, zoom, filter_var, samples, rgba8)
        self._ck(self.L.s2d_render_view_device(self._h, C.byref(cfg), _dev(ptr)))

    def _view_bwd_flags(self, from_target, skip_opacity_grad):
        return (S2D_VIEW_BWD_FROM_TARGET if from_target else 0) | self._bwd_flags(skip_opacity_grad)

    def view_backward_device(self, ptr, out_width, out_height, origin=(0.0, 0.0), zoom=1.0, filter_var=0.0, samples=1,
                             from_target=False, skip_opacity_grad=None):
        """Backward pass through the view (s2d_view_backward_device): from dL/d(view) at `ptr` (device, out_height x out_width
        RGBA32F, 16-byte aligned, .w ignored) -- or, from_target, from a target of the view's size, dL = view - target -- ADDED
        into the gradient buffer, queued on the context's stream; skip_opacity_grad as backward()."""
        cfg = self._view_config(out_width, out_height, origin, zoom, filter_var, samples)
        self._ck(self.L.s2d_view_backward_device(self._h, C.byref(cfg), _dev(ptr), self._view_bwd_flags(from_target, skip_opacity_grad)))

    def view_grads(self, ptr, out_width, out_height, origin=(0.0, 0.0), zoom=1.0, filter_var=0.0, samples=1,
                   from_target=False, skip_opacity_grad=None):
        """The same pass stopped before the adjoint of the record transform: the n gradients of the records view_splats()
        returns (s2d_view_grads); the gradient buffer is not touched."""
        cfg = self._view_config(out_width, out_height, origin, zoom, filter_var, samples)
        a = np.zeros(self.n, dtype=SPLAT_DTYPE)
        self._ck(self.L.s2d_view_grads(self._h, C.byref(cfg), _dev(ptr), self._view_bwd_flags(from_target, skip_opacity_grad), _p(a)))
        return a

    def view_release(self):
        """Frees what views allocated; the next view allocates again."""
        self._ck(self.L.s2d_view_release(self._h))

    def mse(self):
        v = C.c_double()
        self._ck(self.L.s2d_get_mse(self._h, C.byref(v)))
        return v.value

    def sqerr_trace(self, first_iteration, count):
        out = np.zeros(count, dtype=np.float64)
        self._ck(self.L.s2d_get_sqerr_trace(self._h, int(first_iteration), int(count), _p(out)))
        return out

    def synchronize(self):
        self._ck(self.L.s2d_synchronize(self._h))

    # -- multi-GPU plumbing
    def bind_grads(self, device_ptr):
        self._ck(self.L.s2d_bind_grads_device(self._h, _dev(device_ptr)))

    def grads_device_ptr(self):
        return self.L.s2d_grads_device_ptr(self._h)

    # slab ownership (include/splat2d.h, "Slab ownership"): raw DEVICE pointers in, work queued on the context's
    # stream; distributed.HipHaloOps wraps these around torch tensors
    def halo_masks(self, row_bounds, margin_rows, masks_ptr):
        b = (C.c_int32 * len(row_bounds))(*row_bounds)
        self._ck(self.L.s2d_halo_masks(self._h, len(row_bounds) - 1, b, C.c_float(margin_rows), C.c_void_p(masks_ptr)))

    def halo_commit(self, masks_ptr, rank, added=1):
        self._ck(self.L.s2d_halo_commit(self._h, C.c_void_p(masks_ptr), rank, added))

    def rows_gather(self, what, ids_ptr, count, out_ptr):
        self._ck(self.L.s2d_rows_gather(self._h, what, C.c_void_p(ids_ptr), count, C.c_void_p(out_ptr)))

    def rows_scatter(self, what, ids_ptr, count, in_ptr):
        self._ck(self.L.s2d_rows_scatter(self._h, what, C.c_void_p(ids_ptr), count, C.c_void_p(in_ptr)))

    def grads_combine(self, rows_ptr, n_rows, src_ptr, world, recv_ptr):
        self._ck(self.L.s2d_grads_combine(self._h, C.c_void_p(rows_ptr), n_rows, C.c_void_p(src_ptr), world,
                                          C.c_void_p(recv_ptr)))

    # -- diagnostics
    def stats(self):
        s = _Stats()
        s.struct_size = C.sizeof(_Stats)
        self._ck(self.L.s2d_get_stats(self._h, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in _Stats._fields_ if k not in ("struct_size", "reserved")}
        out["bwd_lane_hist"] = list(s.bwd_lane_hist)
        return out

    def rebuild_count(self):
        """Times the tile lists were rebuilt so far (host-side counter: no device synchronisation)."""
        v = C.c_uint64()
        self._ck(self.L.s2d_get_rebuild_count(self._h, C.byref(v)))
        return v.value

    def tile_lists(self):
        st = self.stats()
        tx, ty = C.c_int32(), C.c_int32()
        self._ck(self.L.s2d_debug_get_tile_lists(self._h, C.byref(tx), C.byref(ty), None, 0, None, 0))
        off = np.zeros(tx.value * ty.value + 1, dtype=np.uint32)
        lst = np.zeros(max(int(st["pairs_binned"]), 1), dtype=np.uint32)
        self._ck(self.L.s2d_debug_get_tile_lists(self._h, C.byref(tx), C.byref(ty), _p(off), len(off),
                                                 _p(lst), len(lst)))
        return tx.value, ty.value, off, lst[:int(st["pairs_binned"])]
