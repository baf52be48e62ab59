"""CPU tests of the cutter behind index-range rendering (2dgaussiansplatting_amd/csrc/s2d_ranges.h).

tests/hostcheck/s2d_ranges_check.cpp compiles cut_index_ranges -- the function the library itself calls -- for the host; it
is held to a table of cases here.  The same cutter behind a main() of its own (tests/hostcheck/s2d_ranges_main.cpp) is
built with -fsanitize=address,undefined and run as a child process on the same cases; nothing sanitised is loaded into
Python.

A note on the row [0, 0, 7, 0] with budget 5.  The issue that asked for these tests lists [0, 4] as its result and, in the
same breath, asks for the cutter to hold exactly the loop the library had.  That loop gives [0, 3, 4]: the guard `acc > 0`
keeps a cut from falling in front of the first pair-bearing splat of a range, and nothing else -- behind the 7 the running
count is 7, and 7 + 0 > 5 cuts like any other sum beyond the budget.  The two requirements cannot both hold; this change is a
refactor, so the loop stayed and the expectation here is what the loop (before and after the move) returns.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O

HC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
HEADER = os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc", "s2d_ranges.h")

_shim = None


def cut(counts, budget):
    """cut_index_ranges through the shim (built on demand) -> list of range boundaries."""
    global _shim
    if _shim is None:
        so, src = os.path.join(HC_DIR, "libs2d_ranges_check.so"), os.path.join(HC_DIR, "s2d_ranges_check.cpp")
        if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in (src, HEADER)):
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", so, src])
        _shim = C.CDLL(so)
        _shim.ir_cut.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
        _shim.ir_cut.restype = C.c_int
        _shim.ir_pair_capacity.argtypes = [C.c_uint64]
        _shim.ir_pair_capacity.restype = C.c_uint64
        _shim.ir_max_pairs.restype = C.c_uint64
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    out = np.full(len(c) + 3, -1, dtype=np.int32)
    k = _shim.ir_cut(c.ctypes.data_as(C.c_void_p), len(c), int(budget), out.ctypes.data_as(C.c_void_p))
    assert 2 <= k <= len(c) + 2 and np.all(out[k:] == -1)
    return out[:k].tolist()


def _past_2_32():
    """70 000 splats of 1 .. 131 072 pairs each: about 4.6e9 pairs, more than 32-bit positions address."""
    rng = np.random.default_rng(5)
    c = rng.integers(1, 1 << 17, 70000, dtype=np.uint32)
    c[123] = 0xFFFF0000            # one splat alone is beyond the budget
    assert int(c.astype(np.uint64).sum()) > 1 << 32
    return c


# name -> (counts, budget, expected boundaries or None)
CASES = {
    "three_fives": ([5, 5, 5], 10, [0, 2, 3]),
    "one_splat_over_budget": ([20], 10, [0, 1]),                     # it gets a range of its own
    # acc > 0 guards the cut: none in front of the 7, although 0 + 7 > 5.  The splat behind it is cut off like any other
    # that would not fit (7 + 0 > 5) -- see the module's note on this row.
    "zeros_do_not_cut": ([0, 0, 7, 0], 5, [0, 3, 4]),
    "no_splats": ([], 10, [0, 0]),
    "no_splats_budget_1": ([], 1, [0, 0]),
    "covering_80000": ([1200] * 120, 80000, [0, 66, 120]),           # the numbers in test_gpu_parity.py's comment
    "covering_100000": ([1200] * 120, 100000, [0, 83, 120]),
    "past_2_32": (_past_2_32(), (1 << 32) - 65537, None),
}


def _check_properties(counts, budget, r):
    """What every cut must be: ascending boundaries from 0 to n, no empty range (n > 0), no range beyond the budget unless
    it is a single splat, and no cut that could have come later (the next splat would not have fitted)."""
    c = np.asarray(counts, dtype=np.uint64)
    n = len(c)
    assert r[0] == 0 and r[-1] == n
    if n == 0:
        assert r == [0, 0]
        return
    assert all(a < b for a, b in zip(r, r[1:]))
    for a, b in zip(r, r[1:]):
        total = int(c[a:b].sum())
        assert total <= budget or b - a == 1 or int(c[a:b - 1].sum()) == 0, (a, b, total)
        if b < n:
            assert total + int(c[b]) > budget, (a, b)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cut_index_ranges(name):
    counts, budget, want = CASES[name]
    r = cut(counts, budget)
    if want is not None:
        assert r == want
    _check_properties(counts, budget, r)
    if name == "past_2_32":
        assert [123, 124] in [[a, b] for a, b in zip(r, r[1:])]      # the oversized splat stands alone
        assert len(r) > 3


def test_cut_index_ranges_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The stand-alone program on every case: the shim's boundaries, exit status 0, nothing on stderr."""
    exe = str(tmp_path / "s2d_ranges_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HC_DIR, "s2d_ranges_main.cpp")])
    for name in sorted(CASES):
        counts, budget, _ = CASES[name]
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(src, "wb") as f:
            f.write(struct.pack("<iQ", len(c), budget) + c.tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        raw = open(dst, "rb").read()
        k = struct.unpack_from("<i", raw)[0]
        assert np.frombuffer(raw[4:], dtype="<i4").tolist() == cut(counts, budget) and k * 4 + 4 == len(raw), name


# ---- the growth rule of pair-sized memory (s2d_ranges.h pair_capacity, kMaxPairs) ---------------------------------------------
MAX_PAIRS = 0xFFFF0000


def parent_capacity(need):
    """The expression that stood at each place where pair-sized memory grew before there was one function for it (the context's
    lists and scratch, a view's lists): cap = max(need + need / 4 + 4096, 1 << 16); if (cap > 0xFFFF0000) cap = 0xFFFF0000."""
    return min(max(need + need // 4 + 4096, 1 << 16), 0xFFFF0000)


def pair_capacity(need):
    cut([], 1)  # (loads the shim)
    return int(_shim.ir_pair_capacity(int(need)))


# need -> capacity; 65536 -> 86016 is the first growth of a context that starts with 2^16 pairs (profiles/r08/README.md)
GROWTH_ROWS = [(0, 65536), (1, 65536), (49152, 65536), (49153, 65537), (65536, 86016), (0xFFFF0000 - 1, 0xFFFF0000)]


@pytest.mark.parametrize("need,capacity", GROWTH_ROWS, ids=[str(n) for n, _ in GROWTH_ROWS])
def test_pair_capacity_rows(need, capacity):
    assert parent_capacity(need) == capacity      # the table is the old expression's
    assert pair_capacity(need) == capacity
    assert int(_shim.ir_max_pairs()) == MAX_PAIRS


def test_pair_capacity_is_the_old_expression_monotone_and_sufficient():
    """Powers of two +- 1 up to the bound: the old expression's value, capacity >= need, never beyond the bound, never falling."""
    needs = sorted({min(max((1 << k) + d, 0), MAX_PAIRS - 1) for k in range(33) for d in (-1, 0, 1)} | {49152, 49153, MAX_PAIRS - 1})
    caps = [pair_capacity(n) for n in needs]
    assert caps == [parent_capacity(n) for n in needs]
    assert all(n <= c <= MAX_PAIRS for n, c in zip(needs, caps))
    assert all(a <= b for a, b in zip(caps, caps[1:]))
    assert caps[0] == 1 << 16 and caps[-1] == MAX_PAIRS
