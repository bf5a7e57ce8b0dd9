"""What rtc_occluded_async must write (include/rtc.h), from the CPU oracle alone, and the limit sets of
tests/test_gpu_occluded.py (the GPU's bytes, exactly) and tests/test_occlusion_reference.py (the sets' premises, without a
GPU).  A helper module, not a test.

The definition has two forms, and both are here:
  expected  closest.didHit && closest.dst < L for closest = calculateRayCollision(ray, trianglesOnly)
            (raytracing.c:216-240), from trace_rays_reference.expected
  brute     some primitive's raySphere / rayTriangle (raytracing.c:162-214) reports didHit with dst < L and dst < 999999
The comparison with L is strict, in float32, on the reference's own dst; a NaN limit compares false."""
from __future__ import annotations

import functools

import numpy as np

import oracle.binding as orc
import raytracingc_amd as rt
import trace_rays_reference as tr
from raytracingc_amd._abi import RAY_DT, SPHERE_DT, TRIANGLE_DT

F = np.float32
EPSILON = F(0.001)        # scene.h:37, as a float compare (rtc_device.h kEps)
NO_HIT = F(999999.0)      # HitInfo closest = {0, 999999}
LIMITS = ("none", "inf", "999999", "1e30", "tie", "above", "below", "median", "short", "odd")
ODD = np.array([np.nan, 0.0, -0.0, -1.0, -np.inf, EPSILON, np.nextafter(EPSILON, F(np.inf)), 1e-30], F)
FLAGS = (0, rt.RTC_F_NO_CLUSTER_CULL)


def _f32(tmax, n):
    if tmax is None:
        return np.full(n, np.inf, F)
    t = np.asarray(tmax, F)
    return np.full(n, t, F) if t.ndim == 0 else np.ascontiguousarray(t.reshape(-1))


def expected(tris, spheres, tonly, rays, tmax):
    """bool [n]: (prim != -1) & (depth < tmax), in float32; tmax None: no limit."""
    e = tr.expected(tris, spheres, tonly, rays)
    with np.errstate(all="ignore"):
        return (e["prim"] != -1) & (e["depth"].astype(F) < _f32(tmax, len(e["prim"])))


def primitive_hits(tris, spheres, tonly, rays):
    """(hit bool [n, S + T], dst float32 [n, S + T]): raySphere for every sphere (none with tonly), then rayTriangle for
    every triangle, per ray -- one oracle call per primitive."""
    rays = np.ascontiguousarray(rays, RAY_DT)
    n = len(rays)
    tris = np.zeros(0, TRIANGLE_DT) if tris is None else np.ascontiguousarray(tris, TRIANGLE_DT)
    spheres = np.zeros(0, SPHERE_DT) if spheres is None or tonly else np.ascontiguousarray(spheres, SPHERE_DT)
    hit = np.zeros((n, len(spheres) + len(tris)), bool)
    dst = np.zeros((n, len(spheres) + len(tris)), F)
    with np.errstate(all="ignore"):
        for k in range(len(spheres)):
            h, d, _ = orc.ray_sphere(rays, np.repeat(spheres[k:k + 1], n))
            hit[:, k], dst[:, k] = h != 0, d
        for k in range(len(tris)):
            h, d = orc.ray_triangle(rays, np.repeat(tris[k:k + 1], n))
            hit[:, len(spheres) + k], dst[:, len(spheres) + k] = h != 0, d
    return hit, dst


def brute(tris, spheres, tonly, rays, tmax, hits=None):
    """bool [n]: the first form of the definition.  `hits`: primitive_hits of the same arguments, when the caller has it."""
    hit, dst = hits if hits is not None else primitive_hits(tris, spheres, tonly, rays)
    with np.errstate(all="ignore"):
        return (hit & (dst < _f32(tmax, len(hit))[:, None]) & (dst < NO_HIT)).any(1)


def limits(kind, prim, depth):
    """The limit set `kind` (one of LIMITS) for a ray set whose reference winners and depths are prim, depth: float32 [n],
    or None for `none`."""
    d = np.ascontiguousarray(depth, F)
    n = len(d)
    hit = np.asarray(prim) != -1
    med = F(np.median(d[hit])) if hit.any() else F(1.0)
    with np.errstate(all="ignore"):
        out = {"none": lambda: None, "inf": lambda: np.full(n, np.inf, F), "999999": lambda: np.full(n, NO_HIT, F),
               "1e30": lambda: np.full(n, 1e30, F), "tie": lambda: d.copy(),
               "above": lambda: np.nextafter(d, F(np.inf)), "below": lambda: np.nextafter(d, F(-np.inf)),
               "median": lambda: np.full(n, med, F), "short": lambda: np.full(n, med * F(0.1), F),
               "odd": lambda: np.resize(ODD, n)}[kind]()
    if out is not None:
        out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_limits(kind, name, limit, scale=None, triangles_only=None):
    """limits() of a named set of trace_rays_reference against its own expectation."""
    e = tr.case_expected(kind, name, scale, triangles_only)
    return limits(limit, e["prim"], e["depth"])


@functools.lru_cache(maxsize=None)
def case_occluded(kind, name, limit, scale=None, triangles_only=None):
    """expected() of a named set under a named limit set, from the cached closest hits."""
    e = tr.case_expected(kind, name, scale, triangles_only)
    with np.errstate(all="ignore"):
        out = (e["prim"] != -1) & (e["depth"].astype(F) < _f32(case_limits(kind, name, limit, scale, triangles_only),
                                                              len(e["prim"])))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def segments(name):
    """(RAY_DT [n], tmax float32 [n] == 1): line-of-sight segments from the case's replay rays -- pos unchanged,
    dir = (pos + dir * d) - pos in float32 for a ray that hits at d (the segment ends on the surface: occluded or not by a
    rounding), dir * 1000 for a miss."""
    rays, e = tr.replay(name), tr.case_expected("replay", name)
    hit = e["prim"] != -1
    out = np.zeros(len(rays), RAY_DT)
    with np.errstate(all="ignore"):
        for c in "xyz":
            p, v = rays["pos"][c].astype(F), rays["dir"][c].astype(F)
            end = (p + v * e["depth"].astype(F)).astype(F)
            out["pos"][c] = p
            out["dir"][c] = np.where(hit, (end - p).astype(F), v * F(1000.0))
    out.setflags(write=False)
    lim = np.ones(len(rays), F)
    lim.setflags(write=False)
    return out, lim
