"""Register / LDS / occupancy report of the raster kernels from the gfx950 cross-compile, and its comparison between two trees.

    python tools/kernel_resources.py report [csrc_dir] [unit.hip ...] > new.json (no GPU needed: hipcc -Rpass-analysis=kernel-resource-usage;
                                                                  units: default the raster units, s2d_raster*.hip)
    python tools/kernel_resources.py compare old.json new.json
    python tools/kernel_resources.py asm old_csrc_dir [new_csrc_dir] [unit.hip ...]

compare: every kernel instantiation of `old` must be in `new` with the same SGPRs, VGPRs, AGPRs, scratch, LDS and occupancy
(exit status 1 otherwise); instantiations only `new` has are listed.  A kernel that gained a trailing template flag is
matched with its `false` instantiation (`k<a, b>` of old == `k<a, b, false>` of new), and one that lost a trailing flag
with the old `false` instantiation (`k<a, b, false>` of old == `k<a, b>` of new): adding or dropping a defaulted flag renames
the symbol and must change nothing else.  An instantiation added to a unit has moved the register allocation of unrelated
kernels of that unit before, which is what this is run for.
asm: the device assembly (--offload-device-only -S) of every kernel of the old tree against the same kernel of the new one,
comments dropped and local labels unnumbered: which are instruction for instruction the same (exit status 1 if one is not);
kernels only the new tree has are listed.
The kernels of the named translation units -- by default of every one the build compiles (_build.HIP_SOURCES) -- are pooled per
tree, so a kernel is matched by its name whichever unit holds it; a unit that a tree does not have counts as one without kernels
there, and a kernel name that two units of one tree emit is an error.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}


def _build_flags():
    sys.path.insert(0, ROOT)
    import importlib
    build = importlib.import_module("2dgaussiansplatting_amd._build")
    return build, [f for f in build.HIPCC_FLAGS if f not in ("-shared", "-pthread", "-ldl")]


def _plain(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    return [re.sub(r"\(.*$", "", p).replace("void ", "") for p in out.splitlines()]


def _renamed(new, name):
    """The kernel of `new` that `name` of the old tree became when a trailing template flag was added (its `false`
    instantiation) or a trailing flag that was `false` was dropped."""
    if not name.endswith(">"):
        return None
    got = new.get(name[:-1] + ", false>")
    if got is None and name.endswith(", false>"):
        got = new.get(name[:-len(", false>")] + ">")
    return got


def raster_units():
    return [u for u in _build_flags()[0].HIP_SOURCES if u.startswith("s2d_raster")]


def pooled(what, csrc, units):
    """what = assembly or report: its results for several translation units of one tree as one {kernel: ...}."""
    out, unit_of = {}, {}
    for u in units:
        for name, v in what(csrc, u).items():
            if name in out:
                raise ValueError("%s: emitted by %s and by %s" % (name, unit_of[name], u))
            out[name], unit_of[name] = v, u
    return out


def assembly(csrc, source="s2d_raster.hip"):
    """{kernel: its instructions as text} of one translation unit."""
    build, flags = _build_flags()
    if not os.path.exists(os.path.join(csrc, source)):
        return {}
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        subprocess.run([build.hipcc()] + [f for f in flags if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "--offload-device-only",
                        "-S", os.path.join(csrc, source), "-o", out], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    bodies = {}
    for m in re.finditer(r"^(_ZN3s2d\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        body = re.sub(r"\.L\w+", "L", re.sub(r";.*", "", m.group(2)))
        body = re.sub(r"[ \t]+$", "", body, flags=re.M)  # (the padding in front of a dropped comment depends on the label's digits)
        bodies[m.group(1)] = body.replace(m.group(1), "SELF")
    names = sorted(bodies)
    return {p: bodies[n] for n, p in zip(names, _plain(names))}


def compare_assembly(old, new, label=""):
    same, changed = 0, []
    for name, want in sorted(old.items()):
        got = new.get(name, _renamed(new, name))
        if got == want:
            same += 1
        else:
            changed.append(name)
    print("%s%d of %d kernels of the old tree instruction for instruction the same (%d kernels in the new tree)" % (label, same, len(old), len(new)))
    for n in changed:
        print("  CHANGED: " + n)
    for n in sorted(n for n in new if n not in old and not any(_renamed(new, o) is new[n] for o in old)):
        print("  new: " + n)
    return not changed


def report(csrc, source=None):
    """{kernel: its resources} of one translation unit; without a unit, of the raster units together (pooled)."""
    if source is None:
        return pooled(report, csrc, raster_units())
    build, flags = _build_flags()
    if not os.path.exists(os.path.join(csrc, source)):
        return {}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.hipcc()] + flags + ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(csrc, source), "-o",
                                         os.path.join(tmp, "out.o"), "-Rpass-analysis=kernel-resource-usage"]
        text = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, universal_newlines=True).stderr
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    names = sorted(kernels)
    return {p: kernels[n] for n, p in zip(names, _plain(names))}


def compare(old, new):
    bad, matched = [], 0
    for name, want in sorted(old.items()):
        got = new.get(name, _renamed(new, name))
        if got is None:
            bad.append("%s: gone" % name)
        elif got != want:
            bad.append("%s: %s -> %s" % (name, want, got))
        else:
            matched += 1
    known = set(old) | {n[:-1] + ", false>" for n in old if n.endswith(">")} | {n[:-len(", false>")] + ">" for n in old if n.endswith(", false>")}
    added = sorted(n for n in new if n not in known)
    print("%d of %d kernels of the old tree unchanged, %d new" % (matched, len(old), len(added)))
    for n in added:
        print("  new: %s %s" % (n, new[n]))
    for b in bad:
        print("  CHANGED: " + b)
    return not bad


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "report":
        units = [a for a in sys.argv[2:] if a.endswith(".hip")] or raster_units()  # (as report() without a unit)
        dirs = [a for a in sys.argv[2:] if not a.endswith(".hip")]
        csrc = dirs[0] if dirs else os.path.join(ROOT, "2dgaussiansplatting_amd", "csrc")
        json.dump(pooled(report, csrc, units), sys.stdout, indent=1, sort_keys=True)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(0 if compare(json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))) else 1)
    elif len(sys.argv) >= 3 and sys.argv[1] == "asm":
        dirs = [a for a in sys.argv[3:] if not a.endswith(".hip")]
        units = [a for a in sys.argv[3:] if a.endswith(".hip")] or _build_flags()[0].HIP_SOURCES
        new = dirs[0] if dirs else os.path.join(ROOT, "2dgaussiansplatting_amd", "csrc")
        sys.exit(0 if compare_assembly(pooled(assembly, sys.argv[2], units), pooled(assembly, new, units)) else 1)
    else:
        sys.exit(__doc__)
