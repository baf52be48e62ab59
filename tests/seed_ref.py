"""NumPy restatement of importance-sampled placement (include/splat2d.h, "importance-sampled placement"), written from the
definitions there and not from the kernels: what tests/test_seed_cpu.py and tests/test_gpu_seed.py hold the library to, byte
for byte.  Every float operation is one binary32 operation on float32 arrays, in the order the definitions give; the sums of
the importance are Python / 64-bit integers.  Test infrastructure only.
"""
import numpy as np

F32 = np.float32
U32 = np.uint32
EDGES, ERROR, CALLER = 0, 1, 2
STREAM = 0x5EED5EED
DENOM = F32(4294967296.0)
M32 = 0xFFFFFFFF


def pcg3d(x, y, z):
    """pcg3d (main.cpp:285-292) on uint32 arrays (or scalars), words mod 2^32 -> three uint32 arrays."""
    x = np.atleast_1d(np.asarray(x)).astype(np.uint64) & M32
    y = np.atleast_1d(np.asarray(y)).astype(np.uint64) & M32
    z = np.atleast_1d(np.asarray(z)).astype(np.uint64) & M32
    x, y, z = np.broadcast_arrays(x, y, z)
    x = (x * 1664525 + 1013904223) & M32
    y = (y * 1664525 + 1013904223) & M32
    z = (z * 1664525 + 1013904223) & M32
    x = (x + y * z) & M32
    y = (y + z * x) & M32
    z = (z + x * y) & M32
    x = x ^ (x >> 16)
    y = y ^ (y >> 16)
    z = z ^ (z >> 16)
    x = (x + y * z) & M32
    y = (y + z * x) & M32
    z = (z + x * y) & M32
    return x.astype(U32), y.astype(U32), z.astype(U32)


def round_fp16(img):
    """An RGBA32F image as a context with fp16 images holds it: rounded to nearest even, converted back."""
    return np.asarray(img, dtype=F32).astype(np.float16).astype(F32)


def measure(source, ref=None, image0=None, caller=None):
    """s in [0, 1] of every pixel, (H, W) float32."""
    one = F32(1.0)
    if source == EDGES:
        y = np.asarray(ref, dtype=F32)[..., :3]
        H, W = y.shape[:2]
        xr, xl = np.minimum(np.arange(W) + 1, W - 1), np.maximum(np.arange(W) - 1, 0)
        yd, yu = np.minimum(np.arange(H) + 1, H - 1), np.maximum(np.arange(H) - 1, 0)
        e = np.abs(y[:, xr, :] - y[:, xl, :]) + np.abs(y[yd, :, :] - y[yu, :, :])
        m = (e[..., 0] + e[..., 1]) + e[..., 2]
        return np.minimum(one, m * F32(0.5))
    if source == ERROR:
        d = np.abs(np.asarray(image0, dtype=F32)[..., :3] - np.asarray(ref, dtype=F32)[..., :3])
        m = (d[..., 0] + d[..., 1]) + d[..., 2]
        return np.minimum(one, m * (F32(1.0) / F32(3.0)))
    v = np.asarray(caller, dtype=F32)
    v = np.where(np.isnan(v), F32(0.0), v)
    return np.minimum(one, np.maximum(F32(0.0), v)).astype(F32)


def importance(source, ref=None, image0=None, caller=None, squared=False, floor=0):
    """-> (q (H, W) uint32, total as a Python int)."""
    s = measure(source, ref, image0, caller)
    assert s.dtype == F32
    q0 = (s * F32(4095.0) + F32(0.5)).astype(np.uint64)   # truncation of a value in [0.5, 4095.5]
    if squared:
        q0 = (q0 * q0) >> 12
    q = (q0 + int(floor)).astype(U32)
    return q, int(q.astype(np.uint64).sum())


def draws(ids, seed, total):
    """-> (u: list of Python ints in [0, total), bx, by, az: uint32 arrays) of the rows `ids`."""
    ids = np.asarray(ids, dtype=np.int64)
    ax, ay, az = pcg3d(ids, (2 * int(seed)) & M32, STREAM)
    bx, by, _ = pcg3d(ids, (2 * int(seed) + 1) & M32, STREAM)
    u = [((int(a) << 32 | int(b)) * int(total)) >> 64 for a, b in zip(ax, ay)]
    return u, bx, by, az


def sample(q, u):
    """The smallest pixel whose inclusive prefix sum of q exceeds u, for every u."""
    cum = np.cumsum(np.asarray(q, dtype=np.uint64).reshape(-1))
    return np.searchsorted(cum, np.asarray(u, dtype=np.uint64), side="right")


def clamp(x, lo, hi):
    return np.minimum(np.maximum(x, F32(lo)), F32(hi))  # glm::clamp: max, then min


def scale_of(scale, W, H, n_splats):
    s = F32(scale)
    if s == 0:
        s = np.sqrt(F32(W) * F32(H) / F32(n_splats))
    return clamp(F32(s), 1.0, 1024.0)


def rows(ids, seed, q, total, ref, n_splats, scale=0.0, opacity=0.0):
    """The (len(ids), 9) float32 rows s2d_seed_splats writes for `ids`; None when total == 0 (nothing is written)."""
    if total == 0:
        return None
    H, W = q.shape
    u, bx, by, az = draws(ids, seed, total)
    p = sample(q, u)
    y, x = p // W, p % W
    out = np.zeros((len(p), 9), dtype=F32)
    out[:, 0] = clamp(x.astype(F32) + bx.astype(F32) / DENOM, 0.0, F32(W) - F32(1.0))
    out[:, 1] = clamp(y.astype(F32) + by.astype(F32) / DENOM, 0.0, F32(H) - F32(1.0))
    out[:, 2] = out[:, 3] = scale_of(scale, W, H, n_splats)
    out[:, 4] = F32(3.14159265358979323846) * (az.astype(F32) / DENOM)
    out[:, 5:8] = clamp(np.asarray(ref, dtype=F32)[y, x, :3], 0.0, 1.0)
    out[:, 8] = F32(1.0) if F32(opacity) == 0 else F32(opacity)
    return out


def starved(stats, passes, max_moves, min_weight):
    """Rules 1-2 of csrc/s2d_density.h: the rows with weight / passes < min_weight (in double), ordered by (w, index), the
    first max_moves."""
    st = np.asarray(stats, dtype=F32).reshape(-1, 3)
    if len(st) == 0 or passes <= 0 or max_moves <= 0:
        return np.zeros(0, dtype=np.int32)
    w = st[:, 2].astype(np.float64) / np.float64(passes)
    idx = np.nonzero(w < np.float64(F32(min_weight)))[0]
    order = np.lexsort((idx, w[idx]))
    return idx[order][:int(max_moves)].astype(np.int32)
