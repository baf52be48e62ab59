"""CPU tests of the evidence tooling: what profiles/ is made with must treat the optimistic void launches correctly."""
import csv
import os
import subprocess
import sys

import pytest

import oracle_lib as O

TOOL = os.path.join(O.ROOT, "tools", "profile_summarise.py")


def _write(path, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        w = csv.writer(f)
        w.writerow(["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"])
        w.writerows(rows)


def test_pmc_summaries_average_over_working_launches_only(tmp_path):
    """The first raster kernel of an iteration is launched optimistically and returns at once when the tile lists turn out
    stale: such a launch reads a few per cent of a working launch's counters (or zero traffic) and must not be averaged in.
    Counters whose value does not depend on the work (SQ_WAVES) follow the verdict of the others of their pass; passes are
    separate processes, so launches are told apart pass by pass."""
    k = "void s2d::raster_fused_kernel<false, false>(int)"
    a, b = str(tmp_path / "sq" / "x" / "1_counter_collection.csv"), str(tmp_path / "tr" / "x" / "2_counter_collection.csv")
    rows = []
    for d in range(10):
        void = d in (3, 7)
        for xcd in range(2):   # one row per XCD: added up per dispatch
            rows.append([d, k, "SQ_INSTS_VALU", 10 if void else 500])
            rows.append([d, k, "SQ_WAVES", 100])
    _write(a, rows)
    _write(b, [[100 + d, k, "FETCH_SIZE", 0 if d == 5 else 4000] for d in range(8)])
    out = str(tmp_path / "o.csv")
    subprocess.check_call([sys.executable, TOOL, "pmc", os.path.dirname(os.path.dirname(a)), os.path.dirname(os.path.dirname(b)), out])
    lines = [l for l in open(out).read().splitlines() if not l.startswith("#")]
    hdr, row = lines[0].split(","), lines[1].split(",")
    got = dict(zip(hdr, row))
    assert got["launches"] == "10" and got["working_launches"] == "8"
    assert float(got["SQ_INSTS_VALU"]) == 1000.0      # 2 XCD rows x 500, the two void launches left out
    assert float(got["SQ_WAVES"]) == 200.0
    assert float(got["FETCH_SIZE"]) == 4000.0         # 7 working launches of the other pass


def test_working_launch_durations(tmp_path):
    p = str(tmp_path / "t" / "x" / "1_kernel_trace.csv")
    os.makedirs(os.path.dirname(p))
    with open(p, "w") as f:
        w = csv.writer(f)
        w.writerow(["Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        t = 0
        for d in range(12):
            dur = 20 if d % 4 == 0 else 2000
            w.writerow(["void s2d::raster_fused_kernel<false>(int)", t, t + dur])
            t += dur + 5
    out = str(tmp_path / "w.csv")
    subprocess.check_call([sys.executable, TOOL, "working", str(tmp_path / "t"), out])
    row = [l for l in open(out).read().splitlines() if not l.startswith("#")][1].split(",")
    assert row[1:5] == ["12", "1505", "3", "9"] and float(row[5]) == 2000.0


def test_variant_coverage_names_the_rows_a_trace_never_dispatched(tmp_path):
    """tools/gpu_variant_coverage.py on a synthetic kernel trace: names as rocprofv3 writes them (`void`, the argument list, a
    mangled one, a `.kd` suffix), spread over two files; every row of tests/raster_variants.py but two is dispatched."""
    import raster_variants as RV
    tool = os.path.join(O.ROOT, "tools", "gpu_variant_coverage.py")
    left_out = [RV.NAMES[3], RV.NAMES[-1]]
    stats = [n for n in RV.NAMES if n.endswith(", float*>")]
    assert stats and stats[0] not in left_out
    rows = [["void %s(unsigned int const*, float*)" % n, 10 * k, 10 * k + 5] for k, n in enumerate(RV.NAMES) if n not in left_out]
    rows.append(["void %s(int)" % RV.NAMES[0], 1, 2])                                   # a second dispatch of the first row
    rows.append(["void s2d::raster_backward_kernel<false , false,false, false, false, false, true, float *>(int)", 3, 4])
    rows.append(["_ZN3s2d19gather_grads_kernelEPKjS1_jPKfS1_PjjPf.kd", 5, 6])           # mangled, not a row: information only
    rows.append(["void s2d::adam_kernel<true>(int)", 7, 8])                             # another unit's kernel
    for k, part in enumerate((rows[:40], rows[40:])):
        p = str(tmp_path / "t" / ("p%d" % k) / ("%d_kernel_trace.csv" % k))
        os.makedirs(os.path.dirname(p))
        with open(p, "w") as f:
            w = csv.writer(f)
            w.writerow(["Kernel_Name", "Start_Timestamp", "End_Timestamp"])
            w.writerows(part)
    r = subprocess.run([sys.executable, tool, str(tmp_path / "t")], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1
    lines = r.stdout.splitlines()
    assert lines[0].startswith("# raster kernel variants dispatched: %d of %d " % (len(RV.NAMES) - 2, len(RV.NAMES)))
    got = {l.split(None, 2)[2]: l.split(None, 2)[:2] for l in lines if not l.startswith("#")}
    assert [n for n, v in got.items() if v[0] == "MISSING"] == left_out
    assert got[RV.NAMES[0]] == ["dispatched", "2"]
    assert got["s2d::raster_backward_kernel<false, false, false, false, false, false, true, float*>"] == ["dispatched", "2"]
    assert got["s2d::gather_grads_kernel"] == ["other", "1"] and not any("adam" in n for n in got)
    # ... and with the two rows dispatched as well, every row is there and the exit status says so
    with open(p, "a") as f:
        csv.writer(f).writerows([["void %s()" % n, 0, 1] for n in left_out])
    r = subprocess.run([sys.executable, tool, str(tmp_path / "t")], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and "MISSING" not in r.stdout
    assert r.stdout.startswith("# raster kernel variants dispatched: %d of %d " % (len(RV.NAMES), len(RV.NAMES)))


def test_variant_coverage_reads_the_view_table_too(tmp_path):
    """The same tool with --table view and --table all: the rows of tests/view_variants.py, whose template arguments mix flags
    and a number; a view kernel without a row counts like a missing one; the default stays the raster table."""
    import raster_variants as RV
    import view_variants as VV
    tool = os.path.join(O.ROOT, "tools", "gpu_variant_coverage.py")
    left_out = [VV.NAMES[5], VV.NAMES[-1]]
    rows = [["void %s(unsigned int const*, float4 const*)" % n, 10 * k, 10 * k + 5] for k, n in enumerate(VV.NAMES) if n not in left_out]
    rows.append(["void s2d::view_gradient_kernel<false,1 , false, false,false>(int)", 1, 2])   # a second dispatch, spaced otherwise
    rows.append(["void s2d::view_transform_kernel(float const*, int)", 3, 4])                  # not a row: information only
    rows.append(["_ZN3s2d19view_adjoint_kernelEPKfPKhiNS_9ViewXformES1_Pf.kd", 5, 6])
    rows.append(["void s2d::adam_kernel<true>(int)", 7, 8])
    p = str(tmp_path / "t" / "p0" / "0_kernel_trace.csv")
    os.makedirs(os.path.dirname(p))
    with open(p, "w") as f:
        w = csv.writer(f)
        w.writerow(["Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        w.writerows(rows)

    def run(*table):
        return subprocess.run([sys.executable, tool] + list(table) + [str(tmp_path / "t")], stdout=subprocess.PIPE, universal_newlines=True)

    r = run("--table", "view")
    assert r.returncode == 1
    lines = r.stdout.splitlines()
    assert lines[0].startswith("# view kernel variants dispatched: %d of %d " % (len(VV.NAMES) - 2, len(VV.NAMES)))
    got = {l.split(None, 2)[2]: l.split(None, 2)[:2] for l in lines if not l.startswith("#")}
    assert [n for n, v in got.items() if v[0] == "MISSING"] == left_out
    assert got["s2d::view_gradient_kernel<false, 1, false, false, false>"] == ["dispatched", "2"]
    assert got["s2d::view_transform_kernel"] == ["other", "1"] and got["s2d::view_adjoint_kernel"] == ["other", "1"]
    assert not any("adam" in n for n in got)
    # every row dispatched: exit status 0; a view kernel that has no row: 1 again
    with open(p, "a") as f:
        csv.writer(f).writerows([["void %s()" % n, 0, 1] for n in left_out])
    r = run("--table", "view")
    assert r.returncode == 0 and "MISSING" not in r.stdout and "NO ROW" not in r.stdout
    assert r.stdout.startswith("# view kernel variants dispatched: %d of %d " % (len(VV.NAMES), len(VV.NAMES)))
    r = run()                                                          # the default is the raster table: none of its rows is here
    assert r.returncode == 1 and r.stdout.startswith("# raster kernel variants dispatched: 0 of %d " % len(RV.NAMES))
    r = run("--table", "all")                                          # a section each; the status covers both
    assert r.returncode == 1
    heads = [l for l in r.stdout.splitlines() if "kernel variants dispatched" in l]
    assert len(heads) == 2 and heads[0].startswith("# raster kernel variants dispatched: 0 of ") and \
        heads[1].startswith("# view kernel variants dispatched: %d of %d " % (len(VV.NAMES), len(VV.NAMES)))
    with open(p, "a") as f:
        csv.writer(f).writerows([["void s2d::view_raster_kernel<true, 8, false, false>(int)", 0, 1]])
    r = run("--table", "view")
    assert r.returncode == 1 and "NO ROW" in r.stdout and "MISSING" not in r.stdout
    assert subprocess.run([sys.executable, tool, "--table", "nothing", p], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode != 0


def test_one_residual_correction_gives_the_ieee_quotient():
    """csrc/s2d_walk_backward.h::div_by_recip: q = S*r; q += (S - den*q)*r with r a 1-ulp reciprocal.  What its comment claims, on
    three operand populations of the backward blend's range incl. den = 1e-15 and quotients placed next to rounding midpoints
    (tools/check_recip_division.py, numpy emulation of the fma; the full 3 x 10^8-trial run is profiles/r04/r04_recip_division_check.txt):
    the bare estimate S*r misses the IEEE quotient often, one correction leaves at most a ~1e-7 sliver, and with a correctly
    rounded reciprocal nothing at all."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_recip_division", os.path.join(O.ROOT, "tools", "check_recip_division.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tot = mod.run(total=400_000, procs=1)
    assert set(tot) == {"uniform", "log", "midpoint"}
    for kind, t in tot.items():
        assert t["n"] == 400_000
        for name in mod.NAMES:
            c0, c1, c2, changed_by_second, c3 = t[name]
            assert c0 > 40_000, (kind, name, c0)          # the bare estimate misses the IEEE quotient in > 10 % of the cases
            assert c1 <= 2 and c2 <= c1 + 1 and c3 <= c1 + 1, (kind, name, t[name])
        assert t["r = RN(1/den)"][1] == 0, (kind, t)       # correctly rounded reciprocal: one correction is IEEE division


def test_kernel_resources_pools_units_and_refuses_a_kernel_emitted_twice():
    """tools/kernel_resources.py pooled: the kernels of several units of one tree as one table (a kernel is matched by name
    whichever unit holds it), and a name that two units emit is an error."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(O.ROOT, "tools", "kernel_resources.py"))
    KR = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(KR)
    units = {"a.hip": {"s2d::k<true>": 1}, "b.hip": {"s2d::k<false>": 2}, "c.hip": {"s2d::k<true>": 3}, "gone.hip": {}}
    what = lambda csrc, unit: units[unit]
    assert KR.pooled(what, "csrc", ["a.hip", "gone.hip", "b.hip"]) == {"s2d::k<true>": 1, "s2d::k<false>": 2}
    with pytest.raises(ValueError, match="a.hip and by c.hip"):
        KR.pooled(what, "csrc", ["a.hip", "b.hip", "c.hip"])
