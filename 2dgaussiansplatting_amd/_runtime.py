"""Loading libsplat2d_hip.so: one HIP runtime per process, one library per process, signatures from the table of _abi."""
import ctypes as C
import os
import struct
import warnings

from . import _build
from ._abi import ABI_VERSION, apply_signatures

_lib = None  # the process-wide library: what load_library() without a path returns and new Trainers bind to


def hip_runtimes_mapped():
    """Paths of the HIP runtime images (libamdhip64) mapped into this process."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    except OSError:
        return []


def _elf_dynamic_strings(path, tag):
    """Strings of the given dynamic-section tag (1 = DT_NEEDED, 14 = DT_SONAME) of a 64-bit little-endian ELF file; [] when
    the file cannot be read that way."""
    try:
        with open(path, "rb") as f:
            head = f.read(64)
            if head[:6] != b"\x7fELF\x02\x01":
                return []
            shoff, = struct.unpack_from("<Q", head, 0x28)
            shentsize, shnum = struct.unpack_from("<HH", head, 0x3A)
            f.seek(shoff)
            sh = f.read(shentsize * shnum)
            out = []
            for k in range(shnum):
                _, typ, _, _, off, size, link, _, _, entsize = struct.unpack_from("<IIQQQQIIQQ", sh, k * shentsize)
                if typ != 6:  # SHT_DYNAMIC
                    continue
                _, _, _, _, stroff, strsize, _, _, _, _ = struct.unpack_from("<IIQQQQIIQQ", sh, link * shentsize)
                f.seek(off)
                dyn = f.read(size)
                f.seek(stroff)
                strtab = f.read(strsize)
                for j in range(0, size, 16):
                    t, v = struct.unpack_from("<qQ", dyn, j)
                    if t == tag:
                        out.append(strtab[v:strtab.index(b"\0", v)].decode())
            return out
    except (OSError, struct.error, ValueError):
        return []


def _bind_process_hip_runtime():
    """One HIP runtime per process.

    libsplat2d_hip.so needs `libamdhip64.so.7` (its DT_NEEDED entry, the runtime's SONAME).  PyTorch's ROCm wheel bundles
    its own copy of that runtime as torch/lib/libamdhip64.so -- same SONAME -- and its libraries ask for it as
    `libamdhip64.so`:
      * torch first: the bundled copy is loaded; our DT_NEEDED matches it by SONAME, nothing else is mapped;
      * this library first: the dynamic linker resolves `libamdhip64.so.7` to /opt/rocm/lib, and a later `import torch`
        asks for `libamdhip64.so`, which matches neither the name nor the SONAME of the loaded image, finds the bundled
        file and maps a SECOND runtime: two HSA clients in one process, streams and device pointers of one unknown to
        the other ("torch finds no HIP GPUs").
    So, when no runtime is mapped yet and a PyTorch with a bundled runtime is installed, map THAT file first (by path,
    without importing torch): ours then binds to it by SONAME and a later `import torch` finds the same file.
    S2D_HIP_RUNTIME=system keeps the dynamic linker's choice (a process that never imports torch);
    S2D_HIP_RUNTIME=<path> maps that file.
    """
    if hip_runtimes_mapped():
        return  # a runtime is already in the process: the DT_NEEDED entry binds to it by SONAME
    choice = os.environ.get("S2D_HIP_RUNTIME", "auto")
    if choice == "system":
        return
    path = None
    if choice not in ("auto", "torch"):
        path = choice
    else:
        import importlib.util
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        if spec is not None and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                path = cand
    if path:
        needed = _elf_dynamic_strings(_build.LIB_PATH, 1)  # DT_NEEDED
        soname = _elf_dynamic_strings(path, 14)  # DT_SONAME
        want = [x for x in needed if x.startswith("libamdhip64")]
        if choice in ("auto", "torch") and want and soname and soname[0] not in want:
            # the bundled runtime would not satisfy our DT_NEEDED entry: mapping it would put TWO runtimes into a process
            # that never imports torch and works with the system's alone
            warnings.warn("2dgaussiansplatting_amd: %s has SONAME %s, libsplat2d_hip.so needs %s: leaving the choice of the HIP "
                          "runtime to the dynamic linker (import torch first if this process uses both)" % (path, soname[0], want[0]))
            return
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError as e:
            warnings.warn("2dgaussiansplatting_amd: could not pre-map the HIP runtime %s (%s): leaving the choice to the dynamic "
                          "linker" % (path, e))


def load_library(path=None):
    """dlopen the HIP library.  Raises if it has not been built: there is no fallback.  Without a path: the process-wide
    library, loaded on first use from S2D_LIBRARY or the tree; with one, that file -- which becomes the process-wide library
    only when it is the tree's (use_library makes any other one so)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("S2D_LIBRARY") or _build.LIB_PATH  # S2D_LIBRARY: A/B builds of the same ABI
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the trainer has no CPU fallback)" % path)
    _bind_process_hip_runtime()
    L = C.CDLL(path)
    mapped = hip_runtimes_mapped()
    if len(mapped) > 1:
        raise RuntimeError("two HIP runtimes are mapped into this process (%s): device pointers and streams of one mean "
                           "nothing to the other.  Import this package before anything else loads a differently named "
                           "libamdhip64, or point S2D_HIP_RUNTIME at the runtime the process uses" % ", ".join(mapped))
    ab = path != _build.LIB_PATH  # an A/B build of an older ABI may lack newer entry points (tools/gpu_ab.py)
    if not ab and L.s2d_abi_version() != ABI_VERSION:
        raise RuntimeError("%s was built for ABI version %d, this binding for %d: rebuild it (python -c 'import "
                           "__graft_entry__ as g; g.build()')" % (path, L.s2d_abi_version(), ABI_VERSION))
    apply_signatures(L, lenient=ab)
    if not ab:
        _lib = L
    return L


def use_library(path=None):
    """Makes the library at `path` the process-wide one (tools/gpu_ab*.py alternate between builds of the same ABI); without
    a path the choice is forgotten and the next load_library() loads the default again.  Objects created before keep the
    library they were created with."""
    global _lib
    _lib = None
    if path is not None:
        _lib = load_library(path)
    return _lib
