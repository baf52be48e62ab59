#!/usr/bin/env python3
"""Which raster kernel variants a run dispatched: the measurement that tests/raster_variants.py is true.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python -m pytest -m gpu tests/test_gpu_raster_variants.py
    python tools/gpu_variant_coverage.py <dir or *_kernel_trace.csv> [...] > coverage.txt

Reads the Kernel_Name column of every *_kernel_trace.csv given (a directory is searched for them; one file per process),
brings the names into the form tools/kernel_resources.py prints (demangled, no argument list, no `void`), and lists every
row of the table with the number of its dispatches.  Exit status 1 if a row was never dispatched, or a `s2d::raster_*`
kernel without a row was.  The kernels of the raster units that are no template instantiations (gather_* of s2d_raster_det.hip,
reference_* of s2d_raster_reference.hip, sqerr_finalize) are listed for information only.
"""
import collections
import csv
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFORMATION = re.compile(r"^s2d::(gather_|reference_|sqerr_finalize)")


def table():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import raster_variants
    return raster_variants.NAMES


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


def coverage(files, out=sys.stdout):
    raw = dispatched(files)
    keys = list(raw)
    seen = collections.Counter()
    for key, name in zip(keys, plain(keys)):
        seen[name] += raw[key]
    names = table()
    missing = [n for n in names if seen[n] == 0]
    out.write("# raster kernel variants dispatched: %d of %d (%d trace files, %d dispatches of %d kernels in all)\n"
              % (len(names) - len(missing), len(names), len(files), sum(raw.values()), len(seen)))
    for n in names:
        out.write("%-10s %8d  %s\n" % ("dispatched" if seen[n] else "MISSING", seen[n], n))
    unknown = sorted(n for n in seen if n.startswith("s2d::raster_") and n not in set(names))
    for n in unknown:
        out.write("%-10s %8d  %s\n" % ("NO ROW", seen[n], n))
    out.write("# the other kernels of the raster unit, for information\n")
    for n in sorted(n for n in seen if INFORMATION.match(n)):
        out.write("%-10s %8d  %s\n" % ("other", seen[n], n))
    return missing, unknown


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    missing, unknown = coverage(trace_files(sys.argv[1:]))
    sys.exit(1 if missing or unknown else 0)
