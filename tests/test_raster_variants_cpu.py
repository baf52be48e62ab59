"""The table of raster kernel variants (tests/raster_variants.py) against the compiler's own list: the raster units
(csrc/s2d_raster*.hip) are cross-compiled for gfx950 (no GPU needed) and every `s2d::raster_*` kernel they hold together must
have exactly one row and come out of exactly one unit.  A template flag added to a unit's dispatch makes this fail until its
variants have rows, and with rows they get their test against the oracle (tests/test_gpu_raster_variants.py)."""
import collections
import importlib
import importlib.util
import os

import pytest

import oracle_lib as O
import raster_variants as RV


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
    assert len(RV.ROWS) == len(RV.NAMES) > 0
    for r in RV.ROWS:
        assert r.name.startswith("s2d::" + r.template + "<") and r.entry in RV.ENTRY_POINTS, r
        assert set(r.kw) == {"count_pairs", "fp16_images", "deterministic", "exact_exp", "reference_order"}, r
    # a recipe launches one kernel: no two rows may share theirs
    recipes = collections.Counter((tuple(sorted(r.kw.items())), r.ranges, r.entry, r.skip_opacity_grad, r.density_stats) for r in RV.ROWS)
    assert max(recipes.values()) == 1, [k for k, v in recipes.items() if v > 1]


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed: the raster unit cannot be cross-compiled")
def test_table_equals_the_compiled_raster_kernels():
    KR = _kernel_resources()
    # (without a unit: all raster units together; ValueError for a kernel that two of them emit)
    compiled = {n for n in KR.report(os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc")) if n.startswith("s2d::raster_")}
    twice = sorted(n for n, k in collections.Counter(RV.NAMES).items() if k > 1)
    missing, surplus = sorted(compiled - set(RV.NAMES)), sorted(set(RV.NAMES) - compiled)
    assert not twice and not missing and not surplus, (
        "add or remove a row in tests/raster_variants.py:\n  compiled kernels without a row: %s\n  rows without a compiled kernel: %s\n"
        "  rows that occur twice: %s" % (missing or "none", surplus or "none", twice or "none"))
    assert len(compiled) == len(RV.ROWS)
