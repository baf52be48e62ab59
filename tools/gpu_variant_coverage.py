#!/usr/bin/env python3
"""Which kernel variants a run dispatched: the measurement that tests/raster_variants.py and tests/view_variants.py are true.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python -m pytest -m gpu tests/test_gpu_raster_variants.py
    python tools/gpu_variant_coverage.py [--table raster|view|all] <dir or *_kernel_trace.csv> [...] > coverage.txt

Reads the Kernel_Name column of every *_kernel_trace.csv given (a directory is searched for them; one file per process),
brings the names into the form tools/kernel_resources.py prints (demangled, no argument list, no `void`), and lists every
row of the table with the number of its dispatches.  --table: `raster` (the default) is tests/raster_variants.py, `view` is
tests/view_variants.py, `all` is both, a section each.  Exit status 1 if a row of a chosen table was never dispatched, or a
kernel of its templates (`s2d::raster_*`; `s2d::view_raster_kernel<`, `s2d::view_gradient_kernel<`) without a row was.  The
kernels of the same units that are no template instantiations (gather_* of s2d_raster_det.hip, reference_* of
s2d_raster_reference.hip, sqerr_finalize; view_transform_kernel, view_adjoint_kernel) are listed for information only.
"""
import collections
import csv
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# table: (the helper module of tests/ that holds it, the prefixes of its templates' kernels, the unit's other kernels, what the unit is called)
TABLES = {
    "raster": ("raster_variants", ("s2d::raster_",), re.compile(r"^s2d::(gather_|reference_|sqerr_finalize)"), "raster unit"),
    "view": ("view_variants", ("s2d::view_raster_kernel<", "s2d::view_gradient_kernel<"),
             re.compile(r"^s2d::view_(transform|adjoint)_kernel"), "view units"),
}


def table(which="raster"):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    return __import__(TABLES[which][0]).NAMES


def plain(names):
    """kernel_resources._plain for names as a trace holds them: mangled or not, with or without arguments, a `.kd` suffix."""
    names = [re.sub(r"\.kd$", "", n.strip()) for n in names]
    mangled = sorted({n for n in names if n.startswith("_Z")})
    if mangled:
        out = subprocess.run(["c++filt"], input="\n".join(mangled), check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
        demangled = dict(zip(mangled, out.splitlines()))
        names = [demangled.get(n, n) for n in names]
    out = []
    for n in names:
        n = re.sub(r"\(.*$", "", n).replace("void ", "")
        n = re.sub(r"\s*,\s*", ", ", n)
        out.append(re.sub(r"\s+\*", "*", n).strip())
    return out


def trace_files(paths):
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += sorted(glob.glob(os.path.join(p, "**", "*kernel_trace.csv"), recursive=True))
        else:
            files.append(p)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % " ".join(paths))
    return files


def dispatched(files):
    """{kernel name as the trace has it: dispatches}."""
    raw = collections.Counter()
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                raw[row["Kernel_Name"]] += 1
    return raw


def coverage(files, out=sys.stdout, which="raster"):
    """Writes the section of one table -> (its rows never dispatched, the dispatched kernels of its templates without a row)."""
    raw = dispatched(files)
    keys = list(raw)
    seen = collections.Counter()
    for key, name in zip(keys, plain(keys)):
        seen[name] += raw[key]
    _, prefixes, information, unit = TABLES[which]
    names = table(which)
    missing = [n for n in names if seen[n] == 0]
    out.write("# %s kernel variants dispatched: %d of %d (%d trace files, %d dispatches of %d kernels in all)\n"
              % (which, len(names) - len(missing), len(names), len(files), sum(raw.values()), len(seen)))
    for n in names:
        out.write("%-10s %8d  %s\n" % ("dispatched" if seen[n] else "MISSING", seen[n], n))
    unknown = sorted(n for n in seen if n.startswith(prefixes) and n not in set(names))
    for n in unknown:
        out.write("%-10s %8d  %s\n" % ("NO ROW", seen[n], n))
    out.write("# the other kernels of the %s, for information\n" % unit)
    for n in sorted(n for n in seen if information.match(n)):
        out.write("%-10s %8d  %s\n" % ("other", seen[n], n))
    return missing, unknown


if __name__ == "__main__":
    args = sys.argv[1:]
    which = "raster"
    if args[:1] == ["--table"]:
        if len(args) < 2 or args[1] not in list(TABLES) + ["all"]:
            sys.exit(__doc__)
        which, args = args[1], args[2:]
    if not args:
        sys.exit(__doc__)
    files, bad = trace_files(args), False
    for w in (list(TABLES) if which == "all" else [which]):
        missing, unknown = coverage(files, which=w)
        bad = bad or bool(missing or unknown)
    sys.exit(1 if bad else 0)
