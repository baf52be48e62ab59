"""The rasteriser over a background as a differentiable PyTorch operator (include/splat2d_backdrop.h):

    tb = importlib.import_module("2dgaussiansplatting_amd.torch_backdrop")
    with torch.cuda.stream(torch.cuda.Stream()):
        r = tb.BackdropRenderer(W, H, n)
        img = r.render(splats, background)        # background: (3,) or (H, W, 4) float32 on the renderer's device
        loss(img).backward()                      # splats.grad and background.grad

img = C + T_final * background per pixel and channel (s2d_forward of a context with a backdrop); the gradient of the splats is
the backward walk from dL/d(img) on the composite (s2d_backward_image_grads), the gradient of the background is
s2d_backdrop_grads on the same dL/d(img): T_final * dL/d(img) per pixel for a plane (its .w gets 0), the sums of those terms over
the image for a constant.  A constant's three values are read on the host when it is set, which waits for the stream.

This module imports torch; the package itself does not.
"""
import torch

from .backdrop import BackdropTrainer
from .torch_op import SplatRenderer

__all__ = ["BackdropRenderer"]


class BackdropRenderer(SplatRenderer):
    """A SplatRenderer whose context composites over a background.  render_view() draws over the constant background set last
    (the library refuses a view over a plane, and a view through a backdrop has no gradient)."""

    def __init__(self, width, height, n_splats, **trainer_kw):
        super().__init__(width, height, n_splats, **trainer_kw)
        BackdropTrainer.of(self.trainer)

    def _check_background(self, background):
        ok = (isinstance(background, torch.Tensor) and background.dtype == torch.float32 and background.device == self.device and
              background.is_contiguous() and tuple(background.shape) in ((3,), (self.rows, self.W, 4)))
        if not ok:
            raise ValueError("render() takes the background as a contiguous float32 tensor of shape (3,) or (%d, %d, 4) on %s"
                             % (self.rows, self.W, self.device))

    def _set_background(self, background):
        if background.dim() == 1:
            self.trainer.set_backdrop(background.detach().cpu().numpy())
        else:
            self.trainer.set_backdrop_device(background.data_ptr())
        self.generation += 1  # (image0 is stale: a frame drawn before belongs to another background)

    def render(self, splats, background, density_stats=False):
        """splats as SplatRenderer.render; background (3,) or (H, W, 4) float32 on the renderer's device -> (H, W, 4), .w = 1;
        differentiable with respect to both."""
        self._check_splats("render", splats)
        self._check_background(background)
        return _RenderOver.apply(splats, background, self, bool(density_stats))


class _RenderOver(torch.autograd.Function):
    @staticmethod
    def forward(ctx, splats, background, r, density_stats=False):
        r._check_stream()
        r._set_background(background)
        r._draw(splats)
        img = torch.empty((r.rows, r.W, 4), dtype=torch.float32, device=r.device)
        r.trainer.get_image_rows_device(img.data_ptr())
        ctx.renderer, ctx.generation, ctx.density_stats = r, r.generation, density_stats
        ctx.save_for_backward(splats, background)
        return img

    @staticmethod
    def backward(ctx, grad_image):
        r = ctx.renderer
        splats, background = ctx.saved_tensors
        r._check_stream()
        if ctx.generation != r.generation:  # another frame or another background since: this call's again
            r._set_background(background)
            r._draw(splats)
        g = grad_image.to(torch.float32).contiguous()
        d_splats = d_background = None
        if ctx.needs_input_grad[0]:
            r.grads.zero_()
            r.trainer.backward_image_grads(g.data_ptr(), skip_opacity_grad=False, density_stats=ctx.density_stats)
            d_splats = r.grads[:r.n].clone()
        if ctx.needs_input_grad[1]:
            if background.dim() == 1:
                rgb = r.trainer.backdrop_grads(g.data_ptr(), 0, want_rgb=True)
                d_background = torch.tensor(rgb, dtype=torch.float32, device=r.device)
            else:
                d_background = torch.empty((r.rows, r.W, 4), dtype=torch.float32, device=r.device)
                r.trainer.backdrop_grads(g.data_ptr(), d_background.data_ptr(), want_rgb=False)
        return d_splats, d_background, None, None
