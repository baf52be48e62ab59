"""CPU tests of the list arithmetic of slab ownership (2dgaussiansplatting_amd/csrc/s2d_multi_plan.h): which gradient rows a
rank swaps with which peer, who hands which splat to whom at a refresh, which arrivals come too late, which rows a rank owns.

tests/hostcheck/s2d_multi_plan_check.cpp compiles those functions -- the ones the multi-device handle itself calls -- for the
host.  The exchange plan and the slab rows are held to the Python implementation of the same decisions
(distributed.HaloStep._plan, driven stand-alone on CPU tensors without a process group, and distributed.slab_rows), the
hand-over to the invariants of DESIGN.md section 7, the late count to rows written by hand.  The same calls behind a main()
of their own (tests/hostcheck/s2d_multi_plan_main.cpp) are built with -fsanitize=address,undefined and run as a child
process; nothing sanitised is loaded into Python.
"""
import ctypes as C
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O

D = importlib.import_module("2dgaussiansplatting_amd.distributed")

HC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
HEADER = os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc", "s2d_multi_plan.h")
WORLDS = (1, 2, 3, 8)
SIZES = (0, 1, 40, 1000)

_shim = None


def shim():
    global _shim
    if _shim is None:
        so, src = os.path.join(HC_DIR, "libs2d_multi_plan_check.so"), os.path.join(HC_DIR, "s2d_multi_plan_check.cpp")
        if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in (src, HEADER)):
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", so, src])
        _shim = C.CDLL(so)
        _shim.mp_late.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    return _shim


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _i32(count, fill=-99):
    return np.full(count, fill, dtype=np.int32)


# ---- the five calls through the shim.  Each returns the arrays the stand-alone program writes for the same call, in its order.
def slab_rows(height, rank, world):
    out = _i32(2)
    shim().mp_slab_rows(height, rank, world, _p(out))
    return [out]


def plan(view, rank, world):
    """-> total, n_rows, splits, offsets, send_ids, rows, src (flattened rows x world)"""
    n = len(view)
    splits, offsets, send_ids, rows, src, n_rows = _i32(world), _i32(world), _i32(n * world), _i32(n), _i32(n * world), _i32(1)
    total = shim().mp_plan(_p(np.ascontiguousarray(view, dtype=np.uint32)), n, rank, world, _p(splits), _p(offsets), _p(send_ids), _p(rows), _p(src),
                           _p(n_rows))
    k = int(n_rows[0])
    assert total >= 0 and np.all(send_ids[total:] == -99) and np.all(rows[k:] == -99) and np.all(src[k * world:] == -99)
    return [np.int32([total]), n_rows, splits, offsets, send_ids[:total], rows[:k], src[:k * world]]


def handover(view, fresh, rank, world):
    """-> mask, n_keep, keep, counts, out_ids, out_mask (one segment per destination, in rank order)"""
    n = len(view)
    mask = np.array(view, dtype=np.uint32)
    keep, counts, ids, words = _i32(n), _i32(world), _i32(n * world), np.full(n * world, 0xDEAD, dtype=np.uint32)
    n_keep = shim().mp_handover(_p(mask), _p(np.ascontiguousarray(fresh, dtype=np.uint32)), n, rank, world, _p(keep), _p(counts), _p(ids), _p(words))
    total = int(counts.sum())
    assert n_keep >= 0 and np.all(keep[n_keep:] == -99) and np.all(ids[total:] == -99) and np.all(words[total:] == 0xDEAD)
    return [mask, np.int32([n_keep]), keep[:n_keep], counts, ids[:total], words[:total]]


def merge(mask, held, in_ids, in_mask):
    """-> mask, n_held, held"""
    mask = np.array(mask, dtype=np.uint32)
    room = _i32(len(held) + len(in_ids))
    room[:len(held)] = held
    now = shim().mp_merge(_p(mask), len(mask), _p(room), len(held), _p(np.ascontiguousarray(in_ids, dtype=np.int32)),
                          _p(np.ascontiguousarray(in_mask, dtype=np.uint32)), len(in_ids))
    assert now == len(held) + len(in_ids)
    return [mask, np.int32([now]), room]


def late(rows9, row_begin, row_end):
    sp = np.ascontiguousarray(rows9, dtype=np.float32).reshape(-1, 9)
    return [np.int32([shim().mp_late(_p(sp), len(sp), row_begin, row_end)])]


# ---- inputs
def draws(world, n):
    """name -> the n global hold words of a draw (bit q: rank q holds the splat; never 0)."""
    rng = np.random.default_rng(1000 * world + n)
    out = {"random": rng.integers(1, 1 << world, n, dtype=np.uint32)}
    one_holder = np.uint32(1) << rng.integers(0, world, n).astype(np.uint32)
    out["nothing_shared"] = one_holder                                    # no two ranks share a splat
    if world > 1:
        idle, other = world // 2, (world // 2 + 1) % world
        w = out["random"] & ~np.uint32(1 << idle)
        out["a_rank_holds_nothing"] = np.where(w == 0, np.uint32(1 << other), w).astype(np.uint32)
    out["a_rank_holds_everything"] = (rng.integers(1, 1 << world, n, dtype=np.uint32) | np.uint32(1 << (world - 1))).astype(np.uint32)
    for words in out.values():
        assert words.dtype == np.uint32 and len(words) == n and np.all(words != 0)
    return out


def view_of(words, rank):
    """Rank r's view: word if bit r else 0."""
    return np.where((words >> np.uint32(rank)) & 1, words, 0).astype(np.uint32)


def halo_step_plan(view, rank, world):
    """distributed.HaloStep._plan, stand-alone: CPU tensors, no process group."""
    h = object.__new__(D.HaloStep)
    h.torch, h.rank, h.world, h.dist = torch, rank, world, None
    h.mask = torch.from_numpy(view.astype(np.int32))
    h._plan()
    return h


LATE_ROWS = (64, 128)       # the slab of the hand-written late-count rows


def late_cases():
    """name -> (state rows, expected count) for the slab LATE_ROWS.  reach = 3 * max(sx, sy) + 2 = 8 for sx = 2, sy = 1: every
    sum below is exact in float32, so 'on the edge' is on the edge."""
    def row(y, sx=2.0, sy=1.0):
        return [10.0, y, sx, sy, 0.5, 0.5, 0.5, 0.5, 0.0]
    up, down = np.float32(np.inf), np.float32(-np.inf)
    r0, r1 = np.float32(LATE_ROWS[0]), np.float32(LATE_ROWS[1])
    top, bottom = np.float32(r0 - 8), np.float32(r1 + 8)        # pos.y + reach == row_begin, pos.y - reach == row_end
    return {
        "none": ([], 0),
        "on_the_upper_edge": ([row(top)], 1),
        "one_ulp_above": ([row(np.nextafter(top, down))], 0),
        "on_the_lower_edge": ([row(bottom)], 1),
        "one_ulp_below": ([row(np.nextafter(bottom, up))], 0),
        "reach_from_sy": ([row(top, sx=1.0, sy=2.0)], 1),
        "all_together": ([row(top), row(np.nextafter(top, down)), row(96.0), row(bottom), row(np.nextafter(bottom, up)), row(1000.0)], 3),
    }


# ---- tests
@pytest.mark.parametrize("world", WORLDS)
def test_exchange_plan_is_the_one_halo_step_builds(world):
    for n in SIZES:
        for name, words in draws(world, n).items():
            plans = []
            for r in range(world):
                view = view_of(words, r)
                total, n_rows, splits, offsets, send_ids, rows, src = plan(view, r, world)
                h = halo_step_plan(view, r, world)
                where = (world, n, name, r)
                assert splits.tolist() == h.splits, where
                assert send_ids.tolist() == h.send_ids.tolist(), where
                assert rows.tolist() == h.rows.tolist(), where
                assert src.tolist() == h.src.flatten().tolist(), where
                assert int(total[0]) == sum(h.splits) == len(send_ids) and int(n_rows[0]) == len(rows), where
                assert offsets.tolist() == np.concatenate([[0], np.cumsum(splits)[:-1]]).tolist(), where
                if name == "nothing_shared":
                    assert int(total[0]) == 0, where
                plans.append((splits, offsets, send_ids))
            if name == "a_rank_holds_nothing":
                assert any(not view_of(words, r).any() for r in range(world))
            if name == "a_rank_holds_everything":
                assert any(view_of(words, r).all() for r in range(world)) or n == 0
            for r in range(world):
                for p in range(world):
                    (sr, orr, ir), (sp, op, ip) = plans[r], plans[p]
                    assert sr[p] == sp[r], (world, n, name, r, p)
                    assert ir[orr[p]:orr[p] + sr[p]].tolist() == ip[op[r]:op[r] + sp[r]].tolist(), (world, n, name, r, p)


@pytest.mark.parametrize("world", WORLDS)
def test_hand_over_moves_every_arrival_once_from_its_lowest_holder(world):
    for n in SIZES:
        for name, old in draws(world, n).items():
            fresh = np.random.default_rng(77 * world + n + len(name)).integers(1, 1 << world, n, dtype=np.uint32)
            where = (world, n, name)
            decided = []
            for r in range(world):
                held_before = view_of(old, r) != 0
                decided.append(handover(view_of(old, r), np.where(held_before, fresh, 0), r, world))
            # who hands what to whom: every (splat, newly holding rank) exactly once, from the lowest old holder
            sent = {}
            for r, (_, _, _, counts, ids, words) in enumerate(decided):
                at = 0
                for q in range(world):
                    for i, w in zip(ids[at:at + counts[q]].tolist(), words[at:at + counts[q]].tolist()):
                        assert (i, q) not in sent and w == int(fresh[i]), where
                        sent[(i, q)] = r
                    at += counts[q]
            want = {}
            for i in range(n):
                arriving, lowest = int(fresh[i]) & ~int(old[i]), (int(old[i]) & -int(old[i])).bit_length() - 1
                for q in range(world):
                    if (arriving >> q) & 1:
                        want[(i, q)] = lowest
            assert sent == want, where
            # delivery, in sender order, through the merge
            for q in range(world):
                mask, n_keep, keep, _, _, _ = decided[q]
                in_ids, in_mask = [], []
                for p in range(world):
                    if p == q:
                        continue
                    _, _, _, counts, ids, words = decided[p]
                    at = int(counts[:q].sum())
                    in_ids += ids[at:at + counts[q]].tolist()
                    in_mask += words[at:at + counts[q]].tolist()
                mask, n_held, held = merge(mask, keep, in_ids, in_mask)
                assert mask.tolist() == view_of(fresh, q).tolist(), where + (q,)
                assert held.tolist() == np.flatnonzero(view_of(fresh, q)).tolist(), where + (q,)     # ascending, and exactly that set


@pytest.mark.parametrize("name", sorted(late_cases()))
def test_late_count_at_the_edges(name):
    rows9, want = late_cases()[name]
    assert int(late(rows9, *LATE_ROWS)[0][0]) == want


def test_slab_rows_are_the_rows_of_distributed_slab_rows():
    for height in range(1, 201):
        tile_rows = (height + 15) // 16
        for world in range(1, min(8, tile_rows) + 1):
            for rank in range(world):
                assert tuple(slab_rows(height, rank, world)[0].tolist()) == D.slab_rows(height, rank, world), (height, rank, world)


def test_the_same_calls_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The stand-alone program on every call of the tests above: the shim's answers byte for byte, exit status 0, nothing on stderr."""
    exe = str(tmp_path / "s2d_multi_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HC_DIR, "s2d_multi_plan_main.cpp")])
    asked, expected = [], []

    def record(op, a, b, c, arrays, answer):
        asked.append(struct.pack("<4i", op, a, b, c) + b"".join(np.ascontiguousarray(x).tobytes() for x in arrays))
        expected.append(b"".join(np.ascontiguousarray(x).tobytes() for x in answer))

    for height, world in ((1, 1), (16, 1), (17, 2), (129, 8), (200, 8), (200, 3)):
        for rank in range(world):
            record(1, height, rank, world, [], slab_rows(height, rank, world))
    for world in WORLDS:
        for n in SIZES:
            for name, old in draws(world, n).items():
                fresh = np.random.default_rng(77 * world + n + len(name)).integers(1, 1 << world, n, dtype=np.uint32)
                for r in range(world):
                    view = view_of(old, r)
                    record(2, n, r, world, [view], plan(view, r, world))
                    now = np.where(view != 0, fresh, 0).astype(np.uint32)
                    decided = handover(view, now, r, world)
                    record(3, n, r, world, [view, now], decided)
                    # arrivals for the merge: every splat this rank does not keep, as if handed back to it
                    mask, keep = decided[0], decided[2]
                    in_ids = np.setdiff1d(np.arange(n, dtype=np.int32), keep)[::-1].astype(np.int32)
                    in_mask = fresh[in_ids].astype(np.uint32)
                    record(4, n, len(keep), len(in_ids), [mask, keep, in_ids, in_mask], merge(mask, keep, in_ids, in_mask))
    for name, (rows9, _) in sorted(late_cases().items()):
        sp = np.asarray(rows9, dtype=np.float32).reshape(-1, 9)
        record(5, len(sp), LATE_ROWS[0], LATE_ROWS[1], [sp], late(sp, *LATE_ROWS))
    src, dst = str(tmp_path / "calls.in"), str(tmp_path / "calls.out")
    with open(src, "wb") as f:
        f.write(b"".join(asked))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert open(dst, "rb").read() == b"".join(expected)
