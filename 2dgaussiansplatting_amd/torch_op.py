"""The rasteriser as a differentiable PyTorch operator: any loss written in torch on the rendered image.

    pkg = importlib.import_module("2dgaussiansplatting_amd")
    torch_op = importlib.import_module("2dgaussiansplatting_amd.torch_op")
    with torch.cuda.stream(torch.cuda.Stream()):
        r = torch_op.SplatRenderer(W, H, n)
        splats = torch.nn.Parameter(...)          # (n, 9) float32: pos.xy, sx, sy, rot, color.rgb, opacity (main.cpp:85-93)
        img = r.render(splats)                    # (rows, W, 4) float32, .w = 1 (coverage=True: .w = coverage)
        loss = (img[..., :3] - target).abs().sum()
        loss.backward()                           # splats.grad: the hand-derived backward walk, from dL/d(img)

render_view() is the same for a view of the splats (any zoom, crop and output size, supersampled): s2d_render_view_device
forward, s2d_view_backward_device backward.

Both directions are the library's HIP kernels (s2d_forward, s2d_backward_image_grads) on device pointers of torch's
tensors: nothing crosses the host and nothing synchronises.  The library and torch touch the same buffers, so they work
on ONE stream -- the one that is current when the renderer is created (as distributed.HipHaloOps documents); a call
with another stream current raises.  What the library itself applies to the parameters inside its Adam step (clamps of
the scales, colours and opacity, main.cpp:736-750) is NOT part of render(): a caller's optimiser keeps its parameters in
range itself.

This module imports torch; the package itself does not.
"""
import torch

from .trainer import Trainer

__all__ = ["SplatRenderer"]


class SplatRenderer:
    """A `Trainer` (one GPU, or one row slab: row_begin / row_end in trainer_kw) used as a renderer with a backward pass.

    The context needs a target to run (s2d_forward requires one, and s2d_backward on `trainer` still means the
    reference's loss): the synthetic one is set here; `set_target` replaces it.

    reference_order=True (passed through to the Trainer like every other keyword): the backward walk adds each splat's
    terms in the reference's own order (S2D_CFG_REFERENCE_ORDER), so `splats.grad` is what the reference's loops would
    accumulate from the same dL/d(img), bit for bit -- a validation mode, slower and memory-hungry.

    coverage=True (S2D_CFG_COVERAGE, passed through likewise): .w of render() and render_view() is the coverage of the pixel,
    1 - its final throughput, instead of the constant 1 (255), and the gradient a loss sends into .w of render() reaches
    position, scales, rotation and opacity -- alpha losses, compositing over a background, written in torch.  A view is then
    not differentiable (render_view of a tensor that requires grad raises the library's refusal)."""

    def __init__(self, width, height, n_splats, **trainer_kw):
        if "stream" in trainer_kw:
            raise ValueError("SplatRenderer works on torch's current stream: make the stream current instead of passing it")
        self.device = torch.device("cuda", int(trainer_kw.get("device", torch.cuda.current_device())))
        self.stream = torch.cuda.current_stream(self.device).cuda_stream
        if not self.stream:
            # (a null stream handle in s2d_config means "create one", which torch's work would not be ordered with)
            raise RuntimeError("SplatRenderer cannot share torch's default stream with the library: create it, and call it, "
                               "under `with torch.cuda.stream(torch.cuda.Stream()):`")
        trainer_kw.setdefault("device", self.device.index)
        self.trainer = Trainer(width, height, n_splats, stream=self.stream, **trainer_kw)
        self.n = self.trainer.n
        self.rows, self.W = self.trainer.row_end - self.trainer.row_begin, self.trainer.W
        # the gradient buffer the backward walk accumulates into: torch's memory, zero when bound
        self.grads = torch.zeros((max(self.n, 1), 9), dtype=torch.float32, device=self.device)
        self.trainer.bind_grads(self.grads.data_ptr())
        self.trainer.set_target_synthetic()
        self.generation = 0  # frames drawn so far: image0 and the forward walk's hand-over belong to the last one

    def close(self):
        self.trainer.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_target(self, rgba32f):
        self.trainer.set_target(rgba32f)

    def set_alive(self, mask):
        """Trainer.set_alive: n booleans, False = the row is not drawn and its gradient row comes back as zeros; None: every
        row again.  A frame rendered before the call is drawn again by its backward()."""
        self.trainer.set_alive(mask)
        self.generation += 1

    def alive(self):
        return self.trainer.alive()

    def _check_stream(self):
        if torch.cuda.current_stream(self.device).cuda_stream != self.stream:
            raise RuntimeError("SplatRenderer was created on stream %#x and is called with another stream current: its "
                               "kernels would not be ordered with torch's" % self.stream)

    def _check_splats(self, who, splats):
        if not (isinstance(splats, torch.Tensor) and splats.dtype == torch.float32 and splats.device == self.device and
                tuple(splats.shape) == (self.n, 9) and splats.is_contiguous()):
            raise ValueError("%s() takes a contiguous float32 tensor of shape (%d, 9) on %s" % (who, self.n, self.device))

    def _draw(self, splats):
        """Forward pass of `splats`: afterwards image0 and the hand-over to the backward walk are theirs."""
        self.trainer.set_splats_device(splats.data_ptr())
        self.trainer.forward()
        self.generation += 1

    def render(self, splats, density_stats=False):
        """(n, 9) float32 contiguous tensor on the renderer's device -> the slab's rows of the image, (rows, W, 4), .w = 1 (a coverage
        renderer: .w = coverage); differentiable with respect to `splats`.  density_stats: the backward call of this frame also accumulates the
        density statistics (S2D_BWD_DENSITY_STATS; density() returns them, trainer.relocate() acts on them)."""
        self._check_splats("render", splats)
        return _Render.apply(splats, self, bool(density_stats))

    def render_view(self, splats, out_width, out_height, origin=(0.0, 0.0), zoom=1.0, filter_var=0.0, samples=1, rgba8=False):
        """A view of `splats` (Trainer.render_view: any zoom, crop and output size) -> (out_height, out_width, 4) tensor on
        the renderer's device, float32 with .w = 1 or uint8 with alpha 255 (a coverage renderer: .w = coverage, the alpha
        byte its quantisation).  The parameters are uploaded the way render()
        uploads them, so image0 and the hand-over are theirs afterwards.
        With splats.requires_grad the float view is differentiable with respect to `splats`: its backward is the library's
        pass through the view (s2d_view_backward_device) -- coarse-to-fine, crop and supersampled losses written in torch.  An
        8-bit view has no gradient: rgba8 with requires_grad raises.  Without requires_grad nothing is recorded."""
        self._check_splats("render_view", splats)
        self._check_stream()
        view = (int(out_width), int(out_height), (float(origin[0]), float(origin[1])), float(zoom), float(filter_var), int(samples))
        if splats.requires_grad:
            if rgba8:
                raise ValueError("render_view(rgba8=True) is not differentiable: render the float view of a tensor that requires grad")
            return _RenderView.apply(splats, self, view)
        with torch.no_grad():
            return self._draw_view(splats.detach(), view, rgba8)

    def _draw_view(self, splats, view, rgba8=False):
        self._draw(splats)
        out = torch.empty((view[1], view[0], 4), dtype=torch.uint8 if rgba8 else torch.float32, device=self.device)
        self.trainer.render_view_device(out.data_ptr(), *view, rgba8)
        return out

    def density(self):
        """-> ((n, 3) float32 tensor: sum |dL/dpos.x|, sum |dL/dpos.y|, sum T * alpha per splat over the accumulated
        statistics passes, and the number of those passes); queued on the renderer's stream like everything else."""
        self._check_stream()
        out = torch.empty((max(self.n, 1), 3), dtype=torch.float32, device=self.device)
        passes = self.trainer.density_device(out.data_ptr())
        return out[:self.n], passes

    def density_reset(self):
        self.trainer.density_reset()


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, splats, r, density_stats=False):
        r._check_stream()
        r._draw(splats)
        img = torch.empty((r.rows, r.W, 4), dtype=torch.float32, device=r.device)
        r.trainer.get_image_rows_device(img.data_ptr())
        ctx.renderer, ctx.generation, ctx.density_stats = r, r.generation, density_stats
        ctx.save_for_backward(splats)
        return img

    @staticmethod
    def backward(ctx, grad_image):
        r = ctx.renderer
        (splats,) = ctx.saved_tensors  # (torch raises here if they were modified in place since render())
        r._check_stream()
        if ctx.generation != r.generation:
            # a later render() (or backward) drew another frame: the backward walk needs THIS call's framebuffer and
            # executed entries, so draw its parameters again rather than differentiate the newer frame
            r._draw(splats)
        g = grad_image.to(torch.float32).contiguous()
        r.grads.zero_()
        r.trainer.backward_image_grads(g.data_ptr(), skip_opacity_grad=False, density_stats=ctx.density_stats)
        return r.grads[:r.n].clone(), None, None


class _RenderView(torch.autograd.Function):
    @staticmethod
    def forward(ctx, splats, r, view):
        out = r._draw_view(splats, view)
        ctx.renderer, ctx.view = r, view
        ctx.save_for_backward(splats)
        return out

    @staticmethod
    def backward(ctx, grad_view):
        r = ctx.renderer
        (splats,) = ctx.saved_tensors  # (torch raises here if they were modified in place since render_view())
        r._check_stream()
        # the pass reads the context's CURRENT parameters and needs no frame: upload this call's, which makes image0 and the
        # hand-over of a pending render() stale -- the generation says so, and that call's backward draws its frame again
        r.trainer.set_splats_device(splats.data_ptr())
        r.generation += 1
        g = grad_view.to(torch.float32).contiguous()
        r.grads.zero_()
        r.trainer.view_backward_device(g.data_ptr(), *ctx.view, from_target=False, skip_opacity_grad=False)
        return r.grads[:r.n].clone(), None, None
