"""What rtc_trace_rays_async must write (include/rtc.h), from the CPU oracle alone: each ray through
oracle.binding.calc_path with max_bounce = 1, whose one call is calculateRayCollision(ray, trianglesOnly)
(raytracing.c:216-240) -- first_hit_reference.expected_for's construction for a given ray array -- and the ray sets of
tests/test_gpu_trace_rays.py (the GPU's buffers, bit for bit) and tests/test_trace_rays_reference.py (the sets' premises,
without a GPU).  Every set and every expectation is computed once and is read-only.

The sets, per case (a scene with its camera):
  primary  the 64 x 40 launch's primary rays (tests/primary_rays.launch_rays): first_hit_reference.expected's rays
  replay   that launch rendered by the oracle with seeds x + y * width and maxBounce 10: every calculateRayCollision call
           after a pixel's first, i.e. the bounce rays the renderer really traces, from points on the geometry
  scaled   the replay rays with dir times a factor: 0.25, 3 (|dir|_1 up to ~5.2, beyond the cluster bound's 4), 1e-3, 1e4
  odd      a hand list against the default scene: NaN, infinite, zero, tiny and huge components"""
from __future__ import annotations

import functools

import numpy as np

import chain_path_scenes as cps
import first_hit_reference as fr
import oracle.binding as orc
import raytracingc_amd as rt
from conftest import load_tris, scene_spheres
from primary_rays import launch_rays
from raytracingc_amd._abi import RAY_DT, SPHERE_DT, TRIANGLE_DT

NAMES = fr.NAMES
SHAPE = (64, 40)
# the replay cases and what the oracle gives for them (bounce rays, hits); `default` is the default scene with its sphere
# (trianglesOnly = 0), every other case triangles only
REPLAY = {"suze": (587, 13), "fsuzane": (106, 24), "chunks": (1086, 665), "layers_33": (921, 340),
          "box_diffuse_T": (5009, 5009), "box_mirror": (23040, 23040), "slivers": (1405, 548),
          "mixed_scale": (1120, 164), "nonfinite": (1031, 226), "counts_9": (51, 2), "default": (23033, 23032)}
DEFAULT_SPHERE_HITS = 3124
SCALES = (0.25, 3.0, 1e-3, 1e4)
SCALED_CASES = ("chunks", "layers_33", "slivers")
EXTRA = ("closing_sphere", "open33", "ties_axis", "ties_tilted", "ties_rotated", "tie_scene", "counts_1", "counts_7",
         "counts_8", "counts_9", "counts_63", "counts_64", "counts_65", "layers_16", "layers_17", "layers_32", "layers_33")
OPEN33_RAYS = 4096
RHO_MAX = 4.0  # rtc_layout.h kClusterRhoMax


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(triangles or None, spheres or None, trianglesOnly, camera) of a case."""
    if name == "default":
        return load_tris("default")[0], scene_spheres("default"), 0, rt.camera_basis()
    if name in cps.SCENES:
        tris, cam, _ = cps.SCENES[name]
        return tris, None, 1, cam
    return fr.geometry(name)


def _records(tris, spheres):
    tris = np.zeros(0, TRIANGLE_DT) if tris is None else np.ascontiguousarray(tris, TRIANGLE_DT)
    spheres = np.zeros(0, SPHERE_DT) if spheres is None else np.ascontiguousarray(spheres, SPHERE_DT)
    return tris, spheres


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def expected(tris, spheres, triangles_only, rays):
    """{prim int32 [n], depth float32 [n], normal, albedo float32 [n, 3]}: calculateRayCollision(rays[i], triangles_only)
    in RtcHitBuffers' encoding (+0 on a miss; a triangle's stored normal and colour, a sphere's colour, bit for bit; a
    sphere's normal from the oracle's raySphere)."""
    rays = np.ascontiguousarray(rays, RAY_DT)
    n = len(rays)
    tris, spheres = _records(tris, spheres)
    with np.errstate(all="ignore"):
        _, _, calls, ncalls = orc.calc_path(tris, spheres, rt.default_scene(), int(triangles_only), rays,
                                            np.zeros(n, np.uint32), np.ones(n, np.int32))
    assert (ncalls == 1).all()
    winner, dst = calls[:, 0]["winner"].astype(np.int32), calls[:, 0]["dst"].astype(np.float32)
    normal, albedo = np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32)  # bit patterns: +0 on a miss
    t = winner >= 0
    if t.any():  # the stored normal and the material colour (dwords 9-11 and 12-14 of a Triangle)
        words = tris.view(np.uint32).reshape(len(tris), 17)
        normal[t], albedo[t] = words[winner[t], 9:12], words[winner[t], 12:15]
    s = winner <= -2
    if s.any():  # raySphere's own normal (raytracing.c:181-182); the colour: dwords 4-6 of a Sphere
        which = spheres[-2 - winner[s]]
        hit, sdst, nrm = orc.ray_sphere(rays[s], which)
        assert hit.all() and np.array_equal(sdst.view(np.uint32), dst[s].view(np.uint32))
        normal[s] = nrm.view(np.uint32)
        albedo[s] = spheres.view(np.uint32).reshape(len(spheres), 9)[-2 - winner[s], 4:7]
    return _frozen({"prim": winner, "depth": dst, "normal": normal.view(np.float32), "albedo": albedo.view(np.float32)})


def _config(name):
    return rt.RenderConfig(SHAPE[0], SHAPE[1], 0, 0, bool(geometry(name)[2]))


@functools.lru_cache(maxsize=None)
def primary(name):
    """The 64 x 40 launch's primary rays of a case, RAY_DT [2560]."""
    rays = launch_rays(geometry(name)[3], _config(name))
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def replay_calls(name):
    """The oracle's records (oracle.binding.CALL_DT) of every calculateRayCollision call after a pixel's first, rendering
    the case's 64 x 40 launch with seeds x + y * width and maxBounce 10: the ray, and the winner and dst it must give."""
    tris, spheres, tonly, _ = geometry(name)
    tris, spheres = _records(tris, spheres)
    rays = primary(name)
    n = len(rays)
    with np.errstate(all="ignore"):
        _, _, calls, ncalls = orc.calc_path(tris, spheres, rt.default_scene(), int(tonly), rays,
                                            np.arange(n, dtype=np.uint32), np.full(n, 10, np.int32))
    later = (np.arange(calls.shape[1])[None, :] >= 1) & (np.arange(calls.shape[1])[None, :] < ncalls[:, None])
    out = calls[later].copy()
    out.setflags(write=False)
    return out


def rays_of(calls, scale=1.0):
    """RAY_DT [n] from call records, dir times `scale` (a float32 product per component)."""
    rays = np.zeros(len(calls), RAY_DT)
    with np.errstate(all="ignore"):
        d = (calls["dir"].astype(np.float32) * np.float32(scale)).astype(np.float32)
    for k, c in enumerate("xyz"):
        rays["pos"][c] = calls["pos"][:, k]
        rays["dir"][c] = d[:, k]
    return rays


@functools.lru_cache(maxsize=None)
def replay(name):
    rays = rays_of(replay_calls(name))
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def scaled(name, scale):
    rays = rays_of(replay_calls(name), scale)
    rays.setflags(write=False)
    return rays


def _ray(pos, dir_):
    r = np.zeros(1, RAY_DT)
    for k, c in enumerate("xyz"):
        r["pos"][c], r["dir"][c] = np.float32(pos[k]), np.float32(dir_[k])
    return r


@functools.lru_cache(maxsize=None)
def odd():
    """(RAY_DT [n], labels): the hand list, against the default scene (its camera at the origin looks along +z; the
    sphere's centre from the scene itself)."""
    sph = scene_spheres("default")
    c = tuple(float(sph["pos"][k][0]) for k in "xyz")
    o, z = (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)
    nan, inf = float("nan"), float("inf")
    toward = tuple(np.float32(c[k] - o[k]) for k in range(3))
    rows = [("plain +z", o, z), ("toward the sphere", o, toward),
            ("NaN dir.x", o, (nan, 0.0, 1.0)), ("NaN dir", o, (nan, nan, nan)), ("NaN pos.y", (0.0, nan, 0.0), z),
            ("NaN pos", (nan, nan, nan), toward),
            ("+inf dir.z", o, (0.0, 0.0, inf)), ("-inf dir.x", o, (-inf, 0.0, 1.0)), ("+inf pos.x", (inf, 0.0, 0.0), z),
            ("-inf pos.z", (0.0, 0.0, -inf), z),
            ("dir = 0", o, (0.0, 0.0, 0.0)), ("dir = -0", o, (-0.0, -0.0, -0.0)), ("dir = 0 from the centre", c, (0.0, 0.0, 0.0)),
            ("dir = 0 inside the sphere", (c[0] + 0.01, c[1], c[2]), (0.0, 0.0, 0.0)),
            ("dir 1e-30", o, (0.0, 0.0, 1e-30)), ("dir 1e-20", o, tuple(1e-20 * np.float32(t) for t in toward)),
            ("dir 1e20", o, (0.0, 0.0, 1e20)), ("dir 1e20 toward the sphere", o, tuple(1e20 * np.float32(t) for t in toward)),
            ("dir 3e38", o, (3e38, -3e38, 3e38)),
            ("pos 1e30", (1e30, 0.0, 0.0), (-1.0, 0.0, 0.0)), ("pos 1e30 z", (0.0, 0.0, -1e30), z)]
    with np.errstate(all="ignore"):
        rays = np.concatenate([_ray(p, d) for _, p, d in rows])
    rays.setflags(write=False)
    return rays, tuple(label for label, _, _ in rows)


@functools.lru_cache(maxsize=None)
def case_rays(kind, name, scale=None):
    """The rays of a named set: kind in primary / replay / scaled / odd / extra (an EXTRA scene's 64 x 40 primary rays;
    open33: the 4,096 primary rays of a 128 x 32 launch)."""
    if kind == "primary":
        return primary(name)
    if kind == "replay":
        return replay(name)
    if kind == "scaled":
        return scaled(name, scale)
    if kind == "odd":
        return odd()[0]
    if kind == "extra":
        if name == "open33":
            rays = launch_rays(geometry(name)[3], rt.RenderConfig(128, 32, 0, 0, False))
            assert len(rays) == OPEN33_RAYS
            rays.setflags(write=False)
            return rays
        return primary(name)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def case_expected(kind, name, scale=None, triangles_only=None):
    """expected() of a named set against its case's scene (odd: the default scene; triangles_only None: the case's own)."""
    tris, spheres, tonly, _ = geometry("default" if kind == "odd" else name)
    return expected(tris, spheres, tonly if triangles_only is None else triangles_only, case_rays(kind, name, scale))


def differing(got, want):
    """{buffer: rays whose uint32 bit patterns differ} over the buffers of `got`.  One exception: where an
    expected normal word of a sphere hit is NaN, the result must be NaN, sign and payload free."""
    out = {}
    for k, g in got.items():
        g32, w32 = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)
        d = g32 != w32
        if k == "normal":
            sphere = (np.asarray(want["prim"]) <= -2)[:, None] if "prim" in want else False
            free = sphere & np.isnan(np.ascontiguousarray(want[k]).view(np.float32)) & \
                np.isnan(np.ascontiguousarray(g).view(np.float32))
            d = d & ~free
        out[k] = int((d.any(-1) if d.ndim == 2 else d).sum())
    return out
