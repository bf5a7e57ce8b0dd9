"""The ray order's coherence key (include/rtc.h) restated in numpy float32, operation by operation, and the
designed ray sets of tests/test_ray_order_reference.py (rtc_ray_keys_host against this statement, bit for bit, without a
GPU) and tests/test_gpu_ray_order.py (the device's keys against rtc_ray_keys_host, the device's order against numpy's stable
argsort of them).  Every set is computed once and is read-only."""
from __future__ import annotations

import functools

import numpy as np

from raytracingc_amd._abi import RAY_DT

F = np.float32
# the box most sets use: three different extents, none a power of two away from another
LO = np.array([-3.0, -1.25, 0.5], F)
HI = np.array([5.0, 2.0, 7.25], F)
# a box that is flat on y (hi == lo there: scale 0, every cell 0 on that axis)
FLAT_LO = np.array([-1.0, 2.0, -1.0], F)
FLAT_HI = np.array([1.0, 2.0, 3.0], F)


def scales(lo, hi):
    """scale_a = 32.f / (hi_a - lo_a) when hi_a > lo_a and the quotient is finite, else 0.f."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(all="ignore"):
        q = (F(32) / (hi - lo).astype(F)).astype(F)
    return np.where((hi > lo) & np.isfinite(q), q, F(0)).astype(F)


def _cell(pos, lo, scale):
    with np.errstate(all="ignore"):
        t = ((pos - lo).astype(F) * scale).astype(F)
        c = np.where(t >= F(31), 31, np.where(t >= F(0), np.minimum(t, F(32)), F(0)).astype(np.int64))  # (int)t truncates
    return np.where(t >= F(0), c, 0).astype(np.uint32)                               # !(t >= 0): NaN and below the box


def _q(p):
    with np.errstate(all="ignore"):
        v = (p * F(64)).astype(F)
        c = np.where(v >= F(63), 63, np.where(v >= F(0), np.minimum(v, F(64)), F(0)).astype(np.int64))
    return np.where(p >= F(0), c, 0).astype(np.uint32)


def _spread(c):
    c = c.astype(np.uint32)
    return (c & 1) | (c & 2) << 2 | (c & 4) << 4 | (c & 8) << 6 | (c & 16) << 8


def keys(rays, lo, hi):
    """uint32 [n]: key = cell << 15 | oct << 12 | q(py) << 6 | q(px) of RAY_DT rays in the box lo, hi."""
    r = np.ascontiguousarray(rays, RAY_DT).view(F).reshape(-1, 6)
    lo, sc = np.asarray(lo, F), scales(lo, hi)
    c = [_cell(r[:, a], lo[a], sc[a]) for a in range(3)]
    cell = _spread(c[0]) | _spread(c[1]) << 1 | _spread(c[2]) << 2
    with np.errstate(all="ignore"):
        ax, ay, az = (np.abs(r[:, 3 + a]) for a in range(3))
        L = ((ax + ay).astype(F) + az).astype(F)
        px, py = (ax / L).astype(F), (ay / L).astype(F)
    octant = ((r[:, 3] < 0).astype(np.uint32) | (r[:, 4] < 0).astype(np.uint32) << 1 | (r[:, 5] < 0).astype(np.uint32) << 2)
    return (cell << 15 | octant << 12 | _q(py) << 6 | _q(px)).astype(np.uint32)


def make_rays(pos, dir_):
    """RAY_DT [n] from float32 [n, 3] positions and directions (either may be one row)."""
    pos, dir_ = np.atleast_2d(np.asarray(pos, F)), np.atleast_2d(np.asarray(dir_, F))
    n = max(len(pos), len(dir_))
    out = np.zeros((n, 6), F)
    out[:, :3], out[:, 3:] = pos, dir_
    return out.view(RAY_DT).reshape(-1)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def origin_set():
    """Origins around the edges of the box LO, HI on every axis in turn (the other two coordinates inside): at lo, one ulp
    either side, at hi, one ulp either side, at every cell boundary of the axis (the f32 nearest lo + k (hi - lo) / 32 and
    its two neighbours), far outside, +-inf and NaN; one direction."""
    inside = ((LO + HI) / F(2)).astype(F)
    rows = []
    for a in range(3):
        lo, hi = LO[a], HI[a]
        vals = [lo, np.nextafter(lo, F(-np.inf)), np.nextafter(lo, F(np.inf)), hi, np.nextafter(hi, F(-np.inf)),
                np.nextafter(hi, F(np.inf)), F(-1e30), F(1e30), F(-3e38), F(3e38), F(-np.inf), F(np.inf), F(np.nan),
                F(0), F(-0.0)]
        for k in range(33):
            b = F(lo + F(k) * (hi - lo) / F(32))
            vals += [b, np.nextafter(b, F(-np.inf)), np.nextafter(b, F(np.inf))]
        for v in vals:
            p = inside.copy()
            p[a] = v
            rows.append(p)
    return _frozen(make_rays(np.array(rows, F), [0.3, -0.5, 0.8]))


@functools.lru_cache(maxsize=None)
def flat_set():
    """Origins in and around the box FLAT_LO, FLAT_HI, which has no extent on y: on the plane, either side, NaN, inf."""
    ys = [2.0, np.nextafter(F(2), F(3)), np.nextafter(F(2), F(1)), -7.0, 9.0, np.inf, -np.inf, np.nan]
    pos = [[x, y, z] for y in ys for x in (-1.5, -1.0, 0.0, 0.99, 1.0) for z in (-1.0, 1.0, 2.999, 3.0)]
    return _frozen(make_rays(np.array(pos, F), [-0.2, 0.1, 0.9]))


@functools.lru_cache(maxsize=None)
def direction_set():
    """Directions from one origin inside LO, HI: all 8 octants, +-0 components, p * 64 exactly integral (px = k / 64 with
    py = 0: ax = k, az = 64 - k; and px = py), the zero vector, NaN and inf components, length 1e-30 and 1e30, subnormals."""
    d = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                d += [[sx * 0.2, sy * 0.5, sz * 0.3], [sx * 1.0, sy * 0.0, sz * 0.0], [sx * 0.0, sy * 1.0, sz * 0.0],
                      [sx * 0.0, sy * 0.0, sz * 1.0], [sx * 0.0, sy * 0.0, sz * 0.0], [sx * 3.0, sy * 3.0, sz * 2.0]]
    for k in range(65):
        d += [[k, 0, 64 - k], [0, k, 64 - k], [k, 64 - k, 0], [-k, 0.0, k - 64.0], [k / 2, k / 2, 64 - k]]
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            v = [0.3, -0.4, 0.5]
            v[a] = bad
            d.append(v)
        d.append([bad, bad, bad])
    d += [[np.inf, -np.inf, 1.0], [np.inf, np.inf, np.inf]]
    unit = np.array([0.36, -0.48, 0.8])
    for scale in (1e-30, 1e30, 1e-38, 1e-42, 3e38, 1.0):
        d += [list(unit * scale), list(-unit * scale), [scale, 0, 0], [0, scale, scale]]
    d += [[1e-45, 1e-45, 1e-45], [1e-45, 0, 0], [3e38, 3e38, 3e38], [3e38, -3e38, 1.0]]
    with np.errstate(all="ignore"):
        dirs = np.array(d, np.float64).astype(F)
    return _frozen(make_rays([1.0, 0.0, 3.0], dirs))


@functools.lru_cache(maxsize=None)
def random_set(n=10000, seed=77):
    """Seeded rays: origins in and beyond LO, HI (a margin of a quarter extent), directions of any length."""
    rng = np.random.default_rng(seed)
    ext = (HI - LO).astype(np.float64)
    pos = LO + ext * rng.uniform(-0.25, 1.25, (n, 3))
    dirs = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    return _frozen(make_rays(pos.astype(F), dirs.astype(F)))


DESIGNED = {"origins": (origin_set, LO, HI), "flat": (flat_set, FLAT_LO, FLAT_HI), "directions": (direction_set, LO, HI),
            "random": (random_set, LO, HI)}


def rays_with_keys(wanted):
    """RAY_DT [n] in the box LO, HI whose keys are exactly `wanted` (uint32 [n], each below 2^30): the origin at its
    cell's centre, the direction in its octant with px, py at the centres of their bins (bins with q(px) + q(py) <= 62 only:
    px + py <= 1).  For tests that need chosen key patterns."""
    w = np.asarray(wanted, np.uint32)
    qx, qy, octant, cell = w & 63, (w >> 6) & 63, (w >> 12) & 7, w >> 15
    assert (w < 1 << 30).all() and (qx + qy <= 62).all()
    c = [sum(((cell >> (3 * b + a)) & 1) << b for b in range(5)) for a in range(3)]
    ext = (HI - LO).astype(np.float64)
    pos = np.stack([LO[a] + (c[a] + 0.5) * ext[a] / 32 for a in range(3)], 1)
    px, py = (qx + 0.5) / 64, (qy + 0.5) / 64
    d = np.stack([px, py, 1 - px - py], 1)
    for a in range(3):
        d[:, a] *= np.where((octant >> a) & 1, -1.0, 1.0)
    rays = make_rays(pos.astype(F), d.astype(F))
    assert np.array_equal(keys(rays, LO, HI), w), "the construction must give the keys asked for"
    return rays


def group_share(hit, group=64):
    """The share of `group`-ray groups (consecutive; the last may be short) that hold at least one hitting ray."""
    n = len(hit)
    pad = np.zeros((n + group - 1) // group * group, bool)
    pad[:n] = hit
    return float(pad.reshape(-1, group).any(1).mean())
