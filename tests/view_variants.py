"""The table of view kernel variants: one row per instantiation of the two view templates (csrc/s2d_view.hip view_raster_kernel,
csrc/s2d_view_gradient.hip view_gradient_kernel), with the public recipe that launches it.  A helper module in the style of
tests/raster_variants.py: tests/test_view_variants_cpu.py holds the table to the compiler's own list of kernels,
tests/test_gpu_view_variants.py runs every row against its yardstick, tools/gpu_variant_coverage.py shows from a kernel trace
that every row was dispatched.

The rows are generated from the rules include/splat2d.h, INTEGRATION.md sections 11-13 and DESIGN.md sections 17, 20 and 22
document, not from the C++ dispatch:
  * a view has 1, 2 or 4 samples per axis and RGBA32F or RGBA8 output, with either exponential (splat2d.h, s2d_view_config;
    DESIGN.md section 17);
  * a S2D_CFG_COVERAGE context refuses S2D_CFG_EXACT_EXP at creation and answers S2D_E_INVALID to the view gradient entry
    points; its views carry the coverage in .w or the alpha byte;
  * the gradient through a view is RGBA32F only; its flags are the opacity gradient, deterministic sums and
    S2D_VIEW_BWD_FROM_TARGET (splat2d.h "view gradients");
  * pair counting, reference order and fp16 images add no view variant: a view's own buffers are fp32, a counting or
    reference-order context draws views with the kernels of a plain one and is refused the gradient.
A new template flag needs new rows here: the CPU test fails until the table and the compiler agree again.
"""
import collections
import itertools

ENTRY_POINTS = ("render_view", "view_grads")
SAMPLES = (1, 2, 4)

# name: the demangled kernel as tools/kernel_resources.py prints it.
# kw: Trainer keyword arguments (exact_exp, deterministic, coverage).
# entry: the Trainer method; samples: its argument; rgba8: render_view's (None for view_grads); skip_opacity_grad, from_target:
#     view_grads' (None for render_view).
Row = collections.namedtuple("Row", "name template kw entry samples rgba8 skip_opacity_grad from_target")

BOTH = (False, True)


def _name(template, args):
    return "s2d::%s<%s>" % (template, ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in args))


def _kw(exact=False, det=False, coverage=False):
    return {"exact_exp": exact, "deterministic": det, "coverage": coverage}


def _rows():
    out = []
    # views: deterministic sums are no concern of a forward walk
    for exact, s, rgba8 in itertools.product(BOTH, SAMPLES, BOTH):
        out.append(Row(_name("view_raster_kernel", (exact, s, rgba8, False)), "view_raster_kernel", _kw(exact=exact),
                       "render_view", s, rgba8, None, None))
    # views of a coverage context: no exact exponential
    for s, rgba8 in itertools.product(SAMPLES, BOTH):
        out.append(Row(_name("view_raster_kernel", (False, s, rgba8, True)), "view_raster_kernel", _kw(coverage=True),
                       "render_view", s, rgba8, None, None))
    # gradients through a view: every flag there is; no coverage context, no RGBA8
    for exact, s, op, det, ft in itertools.product(BOTH, SAMPLES, BOTH, BOTH, BOTH):
        out.append(Row(_name("view_gradient_kernel", (exact, s, op, det, ft)), "view_gradient_kernel", _kw(exact=exact, det=det),
                       "view_grads", s, None, not op, ft))
    return out


ROWS = _rows()
NAMES = [r.name for r in ROWS]
TEMPLATES = ("view_raster_kernel", "view_gradient_kernel")


def trainer_kwargs(row):
    """The keyword arguments of Trainer for a row."""
    return {k: v for k, v in row.kw.items() if v}
