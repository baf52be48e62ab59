"""Every raster kernel variant of the dispatch (csrc/s2d_raster.hip launch_raster and the units it hands a pass to) against the oracle: one test per row of
tests/raster_variants.py, the kernel's name as its id.  A row is launched through its public recipe and held to the yardstick
the suite already has for that kind of pass; nothing here is a new tolerance:
  * forward rows: image0 byte-equal to the oracle's (fp16 rows: rounded as test_forward_and_gradients_random_sweep rounds;
    exact rows: the oracle with expf); counting rows also the oracle's counters, as test_forward_bitwise_mini reads them;
  * backward, fused and index-range backward rows: oracle_lib.grad_bars at 1e-4 against backward_stats() on the same
    framebuffer; deterministic rows twice with the same bytes; rows without the opacity gradient leave that column zero (and,
    deterministic, the other eight are the bytes of the row with it); fused deterministic rows give the bytes of forward();
    backward(), their squared error within test_gpu_loss.mse_bound;
  * upstream rows: the masked, signed Charbonnier gradient of tests/test_image_grads_cpu.py, the oracle on its pseudo-target;
  * statistics rows: test_gpu_density.check_against_oracle, and the gradients of the same pass under grad_bars.
One scene for all rows, whose conditions (lists longer than two staging batches with a last batch that is not full, splats
behind the transmittance cut-off, a visible opacity gradient, partial tiles) are asserted once.
tools/gpu_variant_coverage.py shows from a kernel trace that each row launched the kernel it names (profiles/r17).
"""
import functools
import importlib

import numpy as np
import pytest

import oracle_lib as O
import raster_variants as RV
import test_gpu_density as DN
import test_image_grads_cpu as IG
from test_gpu_loss import mse_bound
from test_gpu_parity import REL, _fp16

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
W, H, N, SEED = 100, 50, 700, 3


@functools.lru_cache(maxsize=None)
def scene_inputs():
    return O.synthetic_target(W, H), O.random_splats(N, W, H, SEED)


@functools.lru_cache(maxsize=None)
def oracle_side(exact, fp16, upstream):
    """The oracle's results for one kind of row, computed once and not changed afterwards: the target as the context holds it,
    image0 (fp16 rows: rounded, which is what the backward pass reads), the forward and backward counters, and the gradient
    statistics of the backward pass -- from the reference's loss, or (upstream) from the Charbonnier gradient handed to the
    oracle as its pseudo-target -- plus what the statistics rows compare with."""
    tgt, splats = scene_inputs()
    tgt = _fp16(tgt) if fp16 else tgt
    o = O.OracleTrainer(tgt, N)
    o.splats[:] = splats
    r = {"target": tgt}
    o.L.s2do_set_exact_exp(1 if exact else 0)   # as tests/test_gpu_reference_order.py adversarial_oracle switches it
    try:
        fc, bc = O.Counters(), O.Counters()
        img = o.forward(counters=fc).copy()
        if fp16:
            img = _fp16(img)
            o.image0[:] = img
        r["image"], r["fwd"] = img, (fc.visited, fc.active)
        if upstream:
            g = IG.charbonnier_grad(img, tgt, IG.charbonnier_weights(H, W))
            pseudo = IG.pseudo_target(img, g)   # (fp16 rows: img holds fp16 values, exact in fp32: nothing more to round)
            up = IG.upstream_of(img, pseudo)
            assert (up[..., :3] < 0).any() and (up[..., :3] > 0).any() and not up[:, : W // 3].any()
            r["upstream"] = up
            o.ref = np.ascontiguousarray(pseudo)
        else:
            r["mse"] = o.mse()
        w32, dsum, dabs = o.backward_stats()
        r["w32"], r["dsum"], r["dabs"] = w32.view(np.float32).reshape(-1, 9).copy(), dsum, dabs
        o.ref = tgt
        o.backward(counters=bc)
        r["bwd"] = (bc.visited, bc.active)
        if not exact:
            r["weight"] = DN._weight_from(o)    # sum T * alpha per splat: does not depend on the loss
    finally:
        o.L.s2do_set_exact_exp(0)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def context(fp16=False, **kw):
    t = S2D.Trainer(W, H, N, fp16_images=fp16, **kw)
    t.set_target(oracle_side(False, fp16, False)["target"])
    t.set_splats(scene_inputs()[1].view(S2D.SPLAT_DTYPE))
    return t


@pytest.fixture(scope="module")
def scene():
    """The scene's conditions, asserted once on a plain context; -> the pair budget of the index-range rows."""
    import torch
    torch.zeros(1, device="cuda")                                   # torch's start-up belongs to no row (the upstream rows use it)
    ref = oracle_side(False, False, False)
    with context() as t:
        t.forward()
        pairs = t.stats()["pairs_binned"]
        tx, ty, off, lst = t.tile_lists()
    lengths = np.diff(off.astype(np.int64))
    assert (tx, ty) == (7, 4) and W % 16 and H % 16                 # partial tiles on the right and bottom edges
    assert lengths.max() >= 129, lengths.max()                      # more than two staging batches of 64, four of the deterministic 32
    # The short end.  No list of this scene is shorter than one staging batch (measured on the MI355X: 165 to 390 entries per
    # tile, the bounding circles allow 158 to 391), so that condition cannot be had from these 700 splats; what the walks do
    # at the short end is a last batch that is not full, for the batches of 64 and the deterministic walk's 32 alike.  (The
    # index-range rows walk a quarter of these pairs per range.)
    assert (lengths % 64 != 0).any() and (lengths % 32 != 0).any(), lengths
    assert lengths.min() < lengths.max() // 2, lengths
    assert (ref["dabs"].sum(1) == 0).any()                          # the transmittance cut-off is reached: later entries are skipped
    assert (ref["dabs"][:, 8] > 0).any()                            # a skipped opacity gradient is a visible difference
    assert pairs == len(lst) and pairs // 4 > 0
    return pairs // 4


# ---------------------------------------------------------------------------------------------
# running a row
# ---------------------------------------------------------------------------------------------
def Flags(row):
    return dict(fp16=row.kw["fp16_images"], exact=row.kw["exact_exp"], det=row.kw["deterministic"], count=row.kw["count_pairs"],
                upstream=row.entry == "backward_image_grads")


def launch(row, chunk_pairs):
    """One new context, the row's recipe -> what the pass left: image0, gradients (n, 9), counters, squared error, statistics."""
    f = Flags(row)
    ref = oracle_side(f["exact"], f["fp16"], f["upstream"])
    out = {}
    kw = RV.trainer_kwargs(row, chunk_pairs)
    kw.pop("fp16_images", None)
    with context(f["fp16"], **kw) as t:
        if row.entry != "forward_backward":
            t.forward()
        if row.entry == "backward":
            t.backward(skip_opacity_grad=row.skip_opacity_grad, density_stats=row.density_stats)
        elif row.entry == "forward_backward":
            t.forward_backward(skip_opacity_grad=row.skip_opacity_grad)
        elif row.entry == "backward_image_grads":
            import torch
            u = torch.from_numpy(ref["upstream"].copy()).cuda()
            torch.cuda.synchronize()                                # a plain Trainer works on a stream of its own
            t.backward_image_grads(u.data_ptr(), skip_opacity_grad=row.skip_opacity_grad, density_stats=row.density_stats)
        out["image"] = t.get_image()
        out["stats"] = t.stats()
        if row.entry != "forward":
            out["grads"] = t.get_grads().view(np.float32).reshape(-1, 9).copy()
            if not f["upstream"]:
                out["mse"] = t.mse()
        if row.density_stats:
            out["density"] = t.density()
    return out


@functools.lru_cache(maxsize=None)
def first_launch(name, chunk_pairs):
    """A row's first launch, shared by the rows that compare themselves with it."""
    return launch(ROW[name], chunk_pairs)


ROW = {r.name: r for r in RV.ROWS}


def sibling(row, **changes):
    """The row of the same template whose recipe differs in `changes` (Row fields; kw entries by their Trainer names)."""
    kw = dict(row.kw)
    kw.update({k: v for k, v in changes.items() if k in kw})
    fields = {k: v for k, v in changes.items() if k not in kw}
    want = row._replace(kw=kw, **fields)
    hits = [r for r in RV.ROWS if (r.template, r.kw, r.ranges, r.entry, r.skip_opacity_grad, r.density_stats) ==
            (want.template, want.kw, want.ranges, want.entry, want.skip_opacity_grad, want.density_stats)]
    assert len(hits) == 1, (row.name, changes)
    return hits[0]


def check_forward(row, got, ref):
    assert got["image"].tobytes() == ref["image"].tobytes()
    if row.kw["count_pairs"]:
        assert got["stats"]["fwd_active"] == ref["fwd"][1]          # the same pixels did work
        assert got["stats"]["fwd_visited"] <= ref["fwd"][0]         # tile retirement can only skip visits of dead pixels
        assert got["stats"]["fwd_active"] > 0
    if row.ranges:
        assert got["stats"]["rebins"] >= 3, got["stats"]["rebins"]  # more than two ranges: the carried per-pixel state is used


def check_gradients(row, got, ref):
    w32, dsum, dabs = ref["w32"], ref["dsum"], ref["dabs"]
    if row.skip_opacity_grad:                                       # the column stays zero: grad_bars demands exact zeros where dabs is 0
        assert not got["grads"][:, 8].any()
        w32, dsum, dabs = w32.copy(), dsum.copy(), dabs.copy()
        w32[:, 8] = dsum[:, 8] = dabs[:, 8] = 0
    else:
        assert got["grads"][:, 8].any()
    st = O.grad_bars(got["grads"], w32, dsum, dabs, REL)
    print("\n[variants] %s: %s" % (row.name, {k: "%.3e" % v for k, v in st.items() if k[0] in "abc"}))


# ---------------------------------------------------------------------------------------------
# one test per row
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RV.NAMES)
def test_variant(name, scene):
    row, f = ROW[name], Flags(ROW[name])
    ref = oracle_side(f["exact"], f["fp16"], f["upstream"])
    got = first_launch(name, scene)
    check_forward(row, got, oracle_side(f["exact"], f["fp16"], False))   # every entry point leaves the oracle's image0
    if row.entry == "forward":
        return
    check_gradients(row, got, ref)
    if f["count"]:
        assert got["stats"]["bwd_active"] == ref["bwd"][1] > 0
        assert got["stats"]["bwd_visited"] <= ref["bwd"][0]         # the walk stages only what the forward walk executed
    if f["det"]:
        again = launch(row, scene)
        assert again["grads"].tobytes() == got["grads"].tobytes()
        if row.skip_opacity_grad:
            full = first_launch(sibling(row, skip_opacity_grad=False).name, scene)
            assert full["grads"][:, :8].tobytes() == got["grads"][:, :8].tobytes()
        if row.entry == "forward_backward":
            apart = first_launch(sibling(row, template="raster_backward_kernel", entry="backward", density_stats=False).name, scene)
            assert apart["grads"].tobytes() == got["grads"].tobytes()
            assert abs(got["mse"] - apart["mse"]) <= mse_bound(W, H) * apart["mse"], (got["mse"], apart["mse"])
    if row.density_stats:
        stats, passes = got["density"]
        assert passes == 1 and stats.shape == (N, 3)
        DN.check_against_oracle(row.name, stats, ref["dabs"][:, 0:2], oracle_side(False, f["fp16"], False)["weight"])
