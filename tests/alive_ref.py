"""NumPy restatements of the alive set's rules (include/splat2d.h, "the alive set"): what s2d_prune decides, which rows
s2d_grow picks, and the helpers that turn a scene with a mask into the compact scene the oracle is run on."""
import numpy as np

F32 = np.float32


def prune(alive, stats, passes, opacity, min_weight=0.0, min_opacity=0.0):
    """alive' = alive AND NOT (weight / passes < min_weight [in double, when min_weight > 0] OR opacity < min_opacity [when
    min_opacity > 0]).  stats: (n, 3) float32 density statistics; opacity: n float32.  NaNs prune nothing."""
    alive = np.asarray(alive).astype(bool)
    kill = np.zeros(len(alive), dtype=bool)
    if F32(min_weight) > 0:
        w = np.asarray(stats, dtype=F32).reshape(-1, 3)[:, 2].astype(np.float64)
        with np.errstate(invalid="ignore"):
            kill |= w / np.float64(passes) < np.float64(F32(min_weight))
    if F32(min_opacity) > 0:
        with np.errstate(invalid="ignore"):
            kill |= np.asarray(opacity, dtype=F32) < F32(min_opacity)
    return alive & ~kill


def lowest_dead(alive, count):
    """The min(count, dead) dead rows of lowest index, ascending: what s2d_grow brings to life without explicit ids."""
    dead = np.nonzero(~np.asarray(alive).astype(bool))[0]
    return dead[:max(int(count), 0)].astype(np.int32)


def compact(rows, alive):
    """The rows of the alive splats, in index order (a copy)."""
    return np.ascontiguousarray(np.asarray(rows)[np.asarray(alive).astype(bool)])


def expand(compact_rows, alive, fill):
    """The inverse: an array over all rows with the compact rows at the alive places and `fill` (same shape over all rows)
    elsewhere."""
    out = np.array(fill, copy=True)
    out[np.asarray(alive).astype(bool)] = compact_rows
    return out


def nan_masked(stats, alive):
    """The statistics as s2d_relocate / s2d_reseed hand them to the planners: NaN in every field of a dead row."""
    out = np.array(stats, dtype=F32, copy=True).reshape(-1, 3)
    out[~np.asarray(alive).astype(bool)] = np.nan
    return out


def masks(n, seed=0):
    """The masks of the tests, each over n rows, by name (those that make no sense for n are left out)."""
    rng = np.random.default_rng(1000 + seed)
    m = {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool)}
    one = np.zeros(n, dtype=bool)
    one[n // 2] = True
    m["one"] = one
    second = np.zeros(n, dtype=bool)
    second[::2] = True
    m["every_second"] = second
    if n > 256:
        blk = np.ones(n, dtype=bool)
        blk[:256] = False
        m["first_block_dead"] = blk
    if n > 20:
        last = np.zeros(n, dtype=bool)
        last[-20:] = True
        m["last_20"] = last
    m["random_half"] = rng.random(n) < 0.5
    return m
