"""The table of raster kernel variants: one row per instantiation of the five raster templates of the raster units
(csrc/s2d_raster.hip, s2d_raster_ranges.hip, s2d_raster_gradient.hip; the templates' walks: s2d_walk.h, s2d_walk_backward.h), with
the public recipe that launches it.  A helper module: tests/test_raster_variants_cpu.py holds the table to the compiler's own
list of kernels, tests/test_gpu_raster_variants.py runs every row against the oracle, tools/gpu_variant_coverage.py shows from a
kernel trace that every row was dispatched.

The rows are generated from the rules include/splat2d.h and DESIGN.md document, not from the C++ dispatch:
  * S2D_CFG_EXACT_EXP is not combinable with S2D_CFG_COUNT_PAIRS / S2D_CFG_FP16_IMAGES (splat2d.h);
  * pair counting is a property of the separate forward and backward kernels: the fused launch and index-range rendering have
    no counting variant (splat2d.h, s2d_forward: a counting context answers S2D_E_NOMEM there);
  * s2d_backward_image_grads (UPSTREAM) exists for the two backward kernels that read image0, never with pair counting
    (DESIGN.md section 10);
  * S2D_BWD_DENSITY_STATS exists for the separate backward kernel only, without pair counting and without the exact
    exponential, from the reference's loss or a caller's gradient (splat2d.h);
  * a S2D_CFG_REFERENCE_ORDER context has backward kernels of its own, which are no template variants, and the forward
    kernel of every other context: the flag adds no row.
A new template flag needs new rows here: the CPU test fails until the table and the compiler agree again.
"""
import collections
import itertools

ENTRY_POINTS = ("forward", "backward", "forward_backward", "backward_image_grads")

# name: the demangled kernel as tools/kernel_resources.py prints it.
# kw: Trainer keyword arguments; ranges=True: the context is created with a chunk_pairs below the scene's pair count (the test
#     knows the figure), so the scene is rendered by index ranges.
# entry: the Trainer method; skip_opacity_grad / density_stats: its flags (None where the method has no such flag).
Row = collections.namedtuple("Row", "name template kw ranges entry skip_opacity_grad density_stats")

BOTH = (False, True)


def _name(template, flags, tail=""):
    return "s2d::%s<%s%s>" % (template, ", ".join("true" if f else "false" for f in flags), tail)


def _kw(count=False, half=False, det=False, exact=False, reference_order=False):
    return {"count_pairs": count, "fp16_images": half, "deterministic": det, "exact_exp": exact, "reference_order": reference_order}


def _rows():
    out = []
    # forward passes: deterministic sums and the opacity gradient are no concern of theirs
    for count, half, exact in itertools.product(BOTH, repeat=3):
        if exact and (count or half):
            continue
        out.append(Row(_name("raster_forward_kernel", (count, half, exact)), "raster_forward_kernel",
                       _kw(count=count, half=half, exact=exact), False, "forward", None, None))
    for half, exact in itertools.product(BOTH, repeat=2):
        if exact and half:
            continue
        out.append(Row(_name("raster_forward_chunk_kernel", (half, exact)), "raster_forward_chunk_kernel",
                       _kw(half=half, exact=exact), True, "forward", None, None))
    # the separate backward kernel: every flag there is
    for count, op, half, det, exact, up, stats in itertools.product(BOTH, repeat=7):
        if exact and (count or half):
            continue
        if up and count:
            continue
        if stats and (count or exact):
            continue
        out.append(Row(_name("raster_backward_kernel", (count, op, half, det, exact, up, stats), ", float*" if stats else ""),
                       "raster_backward_kernel", _kw(count=count, half=half, det=det, exact=exact), False,
                       "backward_image_grads" if up else "backward", not op, stats))
    # the fused launch: no counting, no upstream (there is no image yet to have a gradient of), no statistics
    for op, half, det, exact in itertools.product(BOTH, repeat=4):
        if exact and half:
            continue
        out.append(Row(_name("raster_fused_kernel", (op, half, det, exact)), "raster_fused_kernel",
                       _kw(half=half, det=det, exact=exact), False, "forward_backward", not op, None))
    # the backward walk over index ranges: no counting, no statistics
    for op, half, det, exact, up in itertools.product(BOTH, repeat=5):
        if exact and half:
            continue
        out.append(Row(_name("raster_backward_chunk_kernel", (op, half, det, exact, up)), "raster_backward_chunk_kernel",
                       _kw(half=half, det=det, exact=exact), True, "backward_image_grads" if up else "backward", not op, False))
    return out


ROWS = _rows()
NAMES = [r.name for r in ROWS]


def trainer_kwargs(row, chunk_pairs):
    """The keyword arguments of Trainer for a row; chunk_pairs: the pair budget that makes the scene need index ranges."""
    kw = {k: v for k, v in row.kw.items() if v}
    if row.ranges:
        kw["chunk_pairs"] = int(chunk_pairs)
    return kw
