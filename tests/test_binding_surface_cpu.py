"""The Python binding shows its callers what it showed before it was cut into modules: tests/golden/binding_surface.json was
written by tools/make_binding_surface.py on the commit before the cut (the tool's docstring names it), and the tree must
reproduce it -- names and values, method signatures, the argtypes / restype of every symbol, the structures' fields."""
import importlib
import importlib.util
import json
import os

import pytest

import oracle_lib as O

S2D = importlib.import_module("2dgaussiansplatting_amd")


def _tool():
    spec = importlib.util.spec_from_file_location("make_binding_surface", os.path.join(O.ROOT, "tools", "make_binding_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def surfaces():
    S2D._build.build_hip_library()
    tool = _tool()
    return json.load(open(tool.FIXTURE)), tool.surface(S2D), tool


def test_fixture_is_complete(surfaces):
    want, _, tool = surfaces
    assert set(want) == {"names", "methods", "signatures", "structs"}
    assert set(tool.CALLABLES + tool.VALUES + tool.DTYPES + ("_build",)) <= set(want["names"])
    assert len([n for n in want["names"] if n.startswith("S2D_")]) == 19
    assert len(want["signatures"]) == 85 and len(want["structs"]) == 9
    assert set(want["methods"]) == {"Trainer", "MultiTrainer", "SplatRenderer"}
    assert len(want["methods"]["Trainer"]) == 58 and len(want["methods"]["MultiTrainer"]) == 15


def test_module_names_and_values(surfaces):
    want, got, _ = surfaces
    for name, value in want["names"].items():
        assert got["names"].get(name) == value, name
    # what the tree exports beyond the fixture are constants of the header (tests/test_abi_cpu.py holds them to it)
    assert all(n.startswith("S2D_") for n in set(got["names"]) - set(want["names"]))


def test_trainer_and_multi_trainer_methods(surfaces):
    want, got, _ = surfaces
    assert got["methods"]["Trainer"] == want["methods"]["Trainer"]
    assert got["methods"]["MultiTrainer"] == want["methods"]["MultiTrainer"]


def test_signatures_and_structures(surfaces):
    want, got, _ = surfaces
    assert got["signatures"] == want["signatures"]
    assert got["structs"] == want["structs"]


def test_splat_renderer_methods(surfaces):
    pytest.importorskip("torch")
    want, _, tool = surfaces
    got = tool.surface(S2D, importlib.import_module("2dgaussiansplatting_amd.torch_op"))
    assert got["methods"]["SplatRenderer"] == want["methods"]["SplatRenderer"]
