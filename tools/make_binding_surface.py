#!/usr/bin/env python3
"""Writes tests/golden/binding_surface.json: what the Python binding shows its callers.

The fixture is a record of the PARENT of the commit that split the binding into modules: it was written by running this
tool on commit b16f1c1 ("View gradients: backward pass through a view, differentiable render_view"), where the whole
binding was 2dgaussiansplatting_amd/__init__.py, and tests/test_binding_surface_cpu.py holds every later tree to it.  Run
it again only on a commit whose surface is meant to be the new yardstick (a new entry point, a new method), never to make
a failing comparison pass: a fixture taken from the code under test checks nothing.

  python tools/make_binding_surface.py [--check]      (needs the built library; --check prints the differences instead)

It holds
  * names:      the module-level names callers use, with the value of a constant and the `descr` of a dtype;
  * methods:    every public method of Trainer, MultiTrainer and (with torch) torch_op.SplatRenderer with its signature;
  * signatures: per ABI symbol the names of its argtypes and restype as load_library() leaves them;
  * structs:    per ctypes structure the fields' names and type names, and the size.
"""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "binding_surface.json")

CALLABLES = ("Trainer", "MultiTrainer", "S2DError", "load_library", "hip_runtimes_mapped")
VALUES = ("STATUS_NAMES", "ABI_SYMBOLS", "ABI_VERSION", "ROWS_GRADS", "ROWS_SPLATS", "ROWS_ADAM", "OPTIM_GROUPS", "SEED_SOURCES")
DTYPES = ("SPLAT_DTYPE", "ADAM_DTYPE")
STRUCTS = ("_Config", "_Stats", "_SeedConfig", "_ViewConfig", "_OptimConfig", "_LossConfig", "_LossTerms", "_PruneConfig",
           "_RelocateConfig")


def _jsonable(v):
    """A value as json.load returns it: tuples as lists, integer keys as strings."""
    return json.loads(json.dumps(v))


def _methods(cls):
    # (a default that prints with its address, Trainer.set_optim's sentinel, is recorded without it)
    return {name: re.sub(r" at 0x[0-9a-f]+", "", str(inspect.signature(f)))
            for name, f in inspect.getmembers(cls, inspect.isfunction) if not name.startswith("_")}


def _type_name(t):
    return "None" if t is None else t.__name__


def surface(S2D, torch_op=None):
    """The surface of the package S2D (and of its torch_op module when given) as a JSON-ready dict."""
    names = {n: "callable" for n in CALLABLES if callable(getattr(S2D, n))}
    names["_build"] = "module" if inspect.ismodule(S2D._build) else "?"
    names.update({n: getattr(S2D, n) for n in VALUES})
    names["ABI_SYMBOLS"] = sorted(S2D.ABI_SYMBOLS)  # (the order of the list is not part of the surface)
    names.update({n: getattr(S2D, n).descr for n in DTYPES})
    names.update({n: v for n, v in vars(S2D).items() if n.startswith("S2D_") and isinstance(v, int)})
    methods = {"Trainer": _methods(S2D.Trainer), "MultiTrainer": _methods(S2D.MultiTrainer)}
    if torch_op is not None:
        methods["SplatRenderer"] = _methods(torch_op.SplatRenderer)
    L = S2D.load_library()
    # (an unset argtypes and an empty one both mean "no argument": s2d_abi_version)
    signatures = {s: {"argtypes": [_type_name(t) for t in getattr(L, s).argtypes or ()],
                      "restype": _type_name(getattr(L, s).restype)} for s in S2D.ABI_SYMBOLS}
    structs = {n: {"fields": [[f[0], _type_name(f[1])] for f in getattr(S2D, n)._fields_], "size": C.sizeof(getattr(S2D, n))}
               for n in STRUCTS}
    return _jsonable({"names": names, "methods": methods, "signatures": signatures, "structs": structs})


def main():
    sys.path.insert(0, ROOT)
    S2D = importlib.import_module("2dgaussiansplatting_amd")
    got = surface(S2D, importlib.import_module("2dgaussiansplatting_amd.torch_op"))
    if "--check" in sys.argv[1:]:
        want = json.load(open(FIXTURE))
        for part in want:
            for k in sorted(set(want[part]) | set(got[part])):
                if want[part].get(k) != got[part].get(k):
                    print("%s.%s: fixture %r, tree %r" % (part, k, want[part].get(k), got[part].get(k)))
        return
    with open(FIXTURE, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d names, %d symbols" % (FIXTURE, len(got["names"]), len(got["signatures"])))


if __name__ == "__main__":
    main()
