"""Every view kernel variant (csrc/s2d_view.hip launch_view_raster, csrc/s2d_view_gradient.hip launch_view_gradient) against its
yardstick: one test per row of tests/view_variants.py, the kernel's name as its id.  A row is launched through its public recipe
and held to a yardstick the suite already has; nothing here is a new tolerance:
  * view_raster_kernel<EXACT, S, false, false>: the bytes of view_ref.resolve of the oracle's forward loop on the view's records
    at the grid size (out * S), .w = 1 -- the oracle itself, where tests/test_gpu_view.py compares a supersampled view with
    the library's own finer view;
  * <EXACT, S, true, false>: the bytes of view_ref.quantise of the same, on a scene whose colours leave [0, 1] on both sides;
  * <false, S, *, true> (coverage): the white twin of tests/test_gpu_coverage.py, and the plain view it is compared with
    against the oracle as above;
  * view_gradient_kernel, deterministic, caller's upstream: the bytes of a second context of the grid's size
    (view_grad_cases.check_against_second_context), a second call the same bytes;
  * deterministic, from the target: the bytes of the same context's s2d_view_grads fed view - target formed on the device
    (view_grad_cases.check_from_target);
  * float atomics, caller's upstream: oracle_lib.grad_bars against the oracle's backward_stats() at the grid size, the
    Charbonnier upstream of the view pushed through as a pseudo-target (view_grad_cases.oracle_side);
  * float atomics, from the target: the same bars, the target chosen so that the upstream the kernel forms is that Charbonnier
    gradient (view_grad_cases.oracle_side_from_target), after the view the kernel subtracts it from was found to be the
    oracle's in bytes;
  * rows without the opacity gradient: that column zero; deterministic, the other eight are the bytes of the row with it;
    float atomics, the bars after zeroing the column in the oracle's three arrays, as tests/test_gpu_raster_variants.py does.
Scene M through view 1 (output 53 x 37, zoom 2.5: grids 53 x 37, 106 x 74, 212 x 148, partial tiles at every S), whose
conditions are asserted once.  Scene M's lists are long (243 and more entries per tile) and its first two dozen splats
saturate the view, so a second scene (view_ref.scene_sparse, SPARSE_VIEW) runs a subset of the rows at the short end: empty
lists, one entry, fewer than a deterministic staging batch of 32, fewer than a batch of 64, and no pixel behind the cut-off.
tools/gpu_variant_coverage.py shows from a kernel trace that each row launched the kernel it names (profiles/r23).
"""
import functools

import numpy as np
import pytest

import coverage_ref as CR
import oracle_lib as O
import view_grad_cases as VC
import view_ref as V
import view_variants as VV

pytestmark = pytest.mark.gpu

VIEW_OF = {"M": V.VIEWS[0], "Mc": V.VIEWS[0], "S": V.SPARSE_VIEW}
ROW = {r.name: r for r in VV.ROWS}
SPARSE_NAMES = (["s2d::view_raster_kernel<false, %d, false, false>" % s for s in VV.SAMPLES] +
                ["s2d::view_gradient_kernel<false, %d, true, %s, %s>" % (s, d, f) for s in VV.SAMPLES for d in ("false", "true")
                 for f in ("false", "true")] +
                ["s2d::view_gradient_kernel<true, 4, true, true, false>"])
g9 = VC.g9


@functools.lru_cache(maxsize=None)
def oracle_view(name, samples, exact):
    """The view as the oracle draws it, once per case and read-only: the reference's forward loop over the view's records at
    the grid size, resolved in NumPy."""
    origin, zoom, fv, (ow, oh) = VIEW_OF[name]
    rows = V.view_rows(VC.scene(name), origin, zoom, fv, samples)
    img = V.resolve(V.oracle_forward(rows, ow * samples, oh * samples, exact_exp=exact), samples)
    assert np.isfinite(img).all() and np.any(img[..., :3] != 0)
    img.setflags(write=False)
    return img


def list_lengths(name):
    """{samples: the list lengths of the view's grid}, after what every scene is asked: scales the parity tests pin, partial
    tiles on both edges, and an oracle side that is the oracle's view."""
    view = VIEW_OF[name]
    _, _, _, (ow, oh) = view
    out = {}
    for s in VV.SAMPLES:
        VC.assert_pinned(view, s, name)
        assert (ow * s) % 16 and (oh * s) % 16
        for exact in (False, True):
            assert VC.oracle_side(name, view, s, exact)["resolved"].tobytes() == oracle_view(name, s, exact).tobytes()
        out[s] = VC.second_context_list_lengths(name, view, s)
    return out


@pytest.fixture(scope="module")
def scene_m():
    """Scene M does what the rows need, asserted once."""
    import torch
    torch.zeros(1, device="cuda")                                       # torch's start-up belongs to no row
    for s, lengths in list_lengths("M").items():
        print("\n[view variants] scene M x %d: %d tiles, lists of %d to %d entries" % (s, len(lengths), lengths.min(), lengths.max()))
        assert lengths.max() >= 129, lengths                            # more than two staging batches of 64
        assert (lengths % 64 != 0).any() and (lengths % 32 != 0).any(), lengths   # a last batch that is not full, of either size
        for exact in (False, True):
            side = VC.oracle_side("M", VIEW_OF["M"], s, exact)
            assert (side["dabs"][:, 8] > 0).any()                       # a skipped opacity gradient is a visible difference
            assert side["fwd"][1] < side["fwd"][0]                      # the transmittance cut-off is reached: visits that did no work
    return True


@pytest.fixture(scope="module")
def scene_sparse():
    """The sparse scene has the short lists it is there for, asserted once on the lists the library builds."""
    import torch
    torch.zeros(1, device="cuda")
    for s, lengths in list_lengths("S").items():
        print("\n[view variants] sparse scene x %d: %d tiles, %d empty, %d with one entry, longest %d" %
              (s, len(lengths), (lengths == 0).sum(), (lengths == 1).sum(), lengths.max()))
        assert (lengths == 0).any() and (lengths == 1).any(), lengths
        assert ((lengths > 1) & (lengths < 32)).any() and ((lengths >= 33) & (lengths <= 63)).any(), lengths
        assert lengths.max() < 64, lengths                              # no list reaches a whole staging batch
        dabs = VC.oracle_side("S", VIEW_OF["S"], s, False)["dabs"]
        assert (dabs.sum(1) == 0).any() and (dabs.sum(1) > 0).any()     # records without a pixel: their gradients are exact zeros
    return True


# ---------------------------------------------------------------------------------------------
# running a row
# ---------------------------------------------------------------------------------------------
def exp_kw(row):
    return {"exact_exp": True} if row.kw["exact_exp"] else {}


def check_raster(row, name):
    view, s, exact = VIEW_OF[name], row.samples, row.kw["exact_exp"]
    kw = dict(rgba8=row.rgba8, **VC.vkw(view, s))
    if row.kw["coverage"]:
        splats = VC.scene(name)
        twin = CR.white_twin(splats).view(O.SPLAT_DTYPE).reshape(-1)
        with VC.context(splats, coverage=True) as c, VC.context(splats) as p, VC.context(twin) as w:
            vc, vp, vw = (t.render_view(**kw) for t in (c, p, w))
        CR.check_view_against_white_twin(vc, vp, vw, row.rgba8)
        want = oracle_view(name, s, False)                              # ... and the plain view is the oracle's
        assert vp.tobytes() == (V.quantise(want) if row.rgba8 else want).tobytes()
        return
    if row.rgba8:
        assert name == "M"
        want = oracle_view("Mc", s, exact)
        assert want[..., :3].max() > 1 and want[..., :3].min() < 0      # both clamps have work to do
        with VC.context(VC.scene("Mc"), **exp_kw(row)) as t:
            got = t.render_view(**kw)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert got.tobytes() == V.quantise(want).tobytes()
        assert np.all(got[..., 3] == 255) and (got[..., :3] == 255).any() and (got[..., :3] == 0).any()
        assert ((got[..., :3] > 0) & (got[..., :3] < 255)).any()         # ... and there are values to round
        return
    want = oracle_view(name, s, exact)
    with VC.context(VC.scene(name), **exp_kw(row)) as t:
        got = t.render_view(**kw)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert np.all(got[..., 3] == 1)


def check_bars(row, got, side):
    w32, dsum, dabs = side["w32"], side["dsum"], side["dabs"]
    if row.skip_opacity_grad:                                           # the column stays zero: grad_bars demands exact zeros where dabs is 0
        assert not got[:, 8].any()
        w32, dsum, dabs = w32.copy(), dsum.copy(), dabs.copy()
        w32[:, 8] = dsum[:, 8] = dabs[:, 8] = 0
    else:
        assert got[:, 8].any()
    nz = dabs > 0
    print("\n[view variants] %s: gpu vs exact %.3e, oracle fp32 vs exact %.3e (of sum |terms|), gpu vs oracle %.3e"
          % (row.name, (np.abs(got - dsum)[nz] / dabs[nz]).max(), (np.abs(w32 - dsum)[nz] / dabs[nz]).max(),
             (np.abs(got - w32)[nz] / np.maximum(np.abs(w32[nz]), 0.02 * dabs[nz])).max()))
    O.grad_bars(got, w32, dsum, dabs)


def check_gradient(row, name):
    """-> the row's gradients (n, 9), after its asserts."""
    view, s, exact, skip = VIEW_OF[name], row.samples, row.kw["exact_exp"], row.skip_opacity_grad
    if row.kw["deterministic"]:
        if row.from_target:
            got = g9(VC.check_from_target(name, view, s, seed=s, skip=skip, **exp_kw(row))).copy()
        else:
            got = g9(VC.check_against_second_context(name, view, s, skip=skip, **exp_kw(row))).copy()
        if skip:
            full = launch(sibling(row, skip_opacity_grad=False).name, name)
            assert not got[:, 8].any() and full[:, 8].any()
            assert got[:, :8].tobytes() == full[:, :8].tobytes()
        else:
            assert got[:, 8].any()
        return got
    with VC.context(VC.scene(name), **exp_kw(row)) as t:
        if row.from_target:
            side = VC.oracle_side_from_target(name, view, s, exact)
            # the upstream the kernel forms is fp32 (its view - target): its view must be the oracle's for `side` to be its case
            assert t.render_view(**VC.vkw(view, s)).tobytes() == VC.oracle_side(name, view, s, exact)["resolved"].tobytes()
            src = VC.dev(side["target"])
        else:
            side = VC.oracle_side(name, view, s, exact)
            src = VC.dev(side["up"])
        got = g9(t.view_grads(src.data_ptr(), from_target=row.from_target, skip_opacity_grad=skip, **VC.vkw(view, s))).copy()
    check_bars(row, got, side)
    return got


def sibling(row, **changes):
    """The row of the same template whose recipe differs in `changes` (Row fields)."""
    want = row._replace(**changes)
    hits = [r for r in VV.ROWS if r[1:] == want[1:]]
    assert len(hits) == 1, (row.name, changes)
    return hits[0]


@functools.lru_cache(maxsize=None)
def launch(row_name, name):
    """A row on a scene, once: shared with the rows that compare themselves with it."""
    row = ROW[row_name]
    if row.entry == "render_view":
        return check_raster(row, name)
    return check_gradient(row, name)


# ---------------------------------------------------------------------------------------------
# one test per row
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VV.NAMES)
def test_variant(name, scene_m):
    launch(name, "M")


@pytest.mark.parametrize("name", SPARSE_NAMES)
def test_variant_on_short_lists(name, scene_sparse):
    assert name in ROW
    launch(name, "S")
