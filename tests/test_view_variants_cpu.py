"""The table of view kernel variants (tests/view_variants.py) against the compiler's own list: the two view units
(csrc/s2d_view.hip, csrc/s2d_view_gradient.hip) are cross-compiled for gfx950 (no GPU needed) and every
`s2d::view_raster_kernel<` and `s2d::view_gradient_kernel<` they emit must have exactly one row.  A template flag added to
either dispatch makes this fail until its variants have rows, and with rows they get their test
(tests/test_gpu_view_variants.py)."""
import collections
import importlib
import importlib.util
import os

import pytest

import oracle_lib as O
import view_variants as VV

UNITS = {"view_raster_kernel": "s2d_view.hip", "view_gradient_kernel": "s2d_view_gradient.hip"}


def _kernel_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(O.ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _have_hipcc():
    try:
        return bool(importlib.import_module("2dgaussiansplatting_amd._build").hipcc())
    except RuntimeError:
        return False


def test_table_rows_are_well_formed():
    assert len(VV.ROWS) == len(VV.NAMES) > 0 and set(UNITS) == set(VV.TEMPLATES)
    for r in VV.ROWS:
        assert r.name.startswith("s2d::" + r.template + "<") and r.template in VV.TEMPLATES and r.entry in VV.ENTRY_POINTS, r
        assert set(r.kw) == {"exact_exp", "deterministic", "coverage"} and r.samples in VV.SAMPLES, r
        if r.entry == "render_view":
            assert isinstance(r.rgba8, bool) and r.skip_opacity_grad is None and r.from_target is None, r
        else:
            assert r.rgba8 is None and isinstance(r.skip_opacity_grad, bool) and isinstance(r.from_target, bool), r
        assert not (r.kw["coverage"] and (r.kw["exact_exp"] or r.entry == "view_grads")), r   # what a coverage context refuses
    # a recipe launches one kernel: no two rows may share theirs
    recipes = collections.Counter((tuple(sorted(r.kw.items())), r.entry, r.samples, r.rgba8, r.skip_opacity_grad, r.from_target)
                                  for r in VV.ROWS)
    assert max(recipes.values()) == 1, [k for k, v in recipes.items() if v > 1]
    per = collections.Counter(r.template for r in VV.ROWS)
    assert per == {"view_raster_kernel": 12 + 6, "view_gradient_kernel": 48}, per


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed: the view units cannot be cross-compiled")
def test_table_equals_the_compiled_view_kernels():
    KR = _kernel_resources()
    csrc = os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc")
    compiled = []
    for template, unit in UNITS.items():
        compiled += [n for n in KR.report(csrc, unit) if n.startswith("s2d::%s<" % template)]
    assert len(set(compiled)) == len(compiled)
    compiled = set(compiled)
    twice = sorted(n for n, k in collections.Counter(VV.NAMES).items() if k > 1)
    missing, surplus = sorted(compiled - set(VV.NAMES)), sorted(set(VV.NAMES) - compiled)
    assert not twice and not missing and not surplus, (
        "add or remove a row in tests/view_variants.py:\n  compiled kernels without a row: %s\n  rows without a compiled kernel: %s\n"
        "  rows that occur twice: %s" % (missing or "none", surplus or "none", twice or "none"))
    assert len(compiled) == len(VV.ROWS) == 18 + 48
