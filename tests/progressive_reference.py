"""The reference's state between two passes of a progressive frame (rtc_render_samples_async), computed on the
CPU with no code under test in the loop: the primary rays of tests/primary_rays.py (main.c:88-93), one oracle.calc_color
per sample (raytracing.c:262-296: the sample's radiance and the pixel's rngState after it) and numpy float32 arithmetic for
main.c:99, acc = acc + c * (float)(1. / spp) -- the product rounded to float32, then the sum.

reference_pass(...) advances every pixel of a launch by `count` samples from the incoming (accum, rng) -- None: the frame's
start, rng = x + y * width (main.c:95) and accum = +0 -- and returns (accum, rng, colors, segments): the reference's
accumulatedColor and rngState after first + count iterations, vec3ToColor of that sum (raytracing.c:11-15) and the pass's
calculateRayCollision calls.  calc_color does not report its calls, so they are derived per sample: the hits h are the
7-draw steps (6 with calcDebugColor) between the state before and after, and the sample made one more call exactly when it
ended on a miss.  calcColor ends on a miss exactly when the environment enters its light, which a second calc_color from
the same state with a sky 10^10 times brighter shows (the path does not depend on the sky; a path alive at a miss has a
throughput component of 1 after the roulette's division, or is the primary ray); calcDebugColor leaves its loop early
only on a miss (h < maxBounce).  tests/test_progressive_reference.py checks the whole of it against oracle.render."""
from __future__ import annotations

import ctypes as C
import functools
import hashlib
import types

import numpy as np

import oracle.binding as orc
from primary_rays import launch_rays, launch_rows
from raytracingc_amd._abi import RTC_F_DEBUG_BOUNCES, Scene, Vec3

F = np.float32
LCG_A, LCG_C = np.uint32(747796405), np.uint32(2891336453)  # moremath.c:89-95 (RandomValue's state step)


def _launch(desc):
    """The launch's shape as primary_rays wants it (a RenderConfig's attribute names)."""
    n = orc.lib().oracle_rows_selected(C.byref(desc))
    return types.SimpleNamespace(width=desc.width, height=desc.height, row_start=desc.rowStart, row_stride=desc.rowStride,
                                 row_band=desc.rowBand, rows=lambda: n)


def seeds(desc):
    """main.c:95: rngState = x + y * width for every pixel of the launch (pixel = launch row * width + x)."""
    L = _launch(desc)
    y = np.repeat(launch_rows(L), desc.width).astype(np.int64)
    x = np.tile(np.arange(desc.width), L.rows()).astype(np.int64)
    return ((x + y * desc.width) & 0xFFFFFFFF).astype(np.uint32)


def advance(state, draws):
    s = state.copy()
    with np.errstate(over="ignore"):
        for _ in range(draws):
            s = s * LCG_A + LCG_C
    return s


def hits_between(before, after, per_hit, max_hits):
    """How many hits (per_hit draws each) take `before` to `after`."""
    h = np.full(len(before), -1, np.int64)
    s = before.copy()
    for j in range(max_hits + 1):
        h[(h < 0) & (s == after)] = j
        s = advance(s, per_hit)
    assert (h >= 0).all(), "a sample's state is not a whole number of hits past its start"
    return h


def bright_sky(scene: Scene) -> Scene:
    b = Scene()
    C.memmove(C.byref(b), C.byref(scene), C.sizeof(Scene))
    b.skyColorHorizon = b.skyColorZenith = b.groundColor = Vec3(1e10, 1e10, 1e10)
    return b


def to_color(acc):
    """vec3ToColor / floatToUint (raytracing.c:11-15, moremath.c:25-30): < 0 -> 0, >= 1 -> 255, NaN -> 0, else the f32
    product with 255 truncated."""
    with np.errstate(invalid="ignore"):
        v = (acc * F(255)).astype(F)
        out = np.where(acc >= 1, 255, np.where((acc < 0) | np.isnan(acc), 0, np.nan_to_num(v, nan=0.0, posinf=0.0)))
    return out.astype(np.int64).astype(np.uint8)


def sample(tris, spheres, scene, desc, rays, state, cache=None):
    """One iteration of main.c:98 for every pixel: (radiance float32 [n, 3], state after, calculateRayCollision calls, hits).
    `cache` (a dict of one scene, camera and launch shape; results are read-only): the same states are not traced twice."""
    if cache is not None:
        key = (hashlib.sha1(state.tobytes()).hexdigest(), desc.maxBounce, desc.flags & RTC_F_DEBUG_BOUNCES)
        if key not in cache:
            cache[key] = sample(tris, spheres, scene, desc, rays, state)
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]
    debug = bool(desc.flags & RTC_F_DEBUG_BOUNCES)
    mb = np.full(len(rays), desc.maxBounce, np.int32)
    rad, after = orc.calc_color(tris, spheres, scene, desc.trianglesOnly, rays, state, mb, debug)
    hits = hits_between(state, after, 6 if debug else 7, max(desc.maxBounce, 0))
    if desc.maxBounce <= 0:
        return rad, after, np.zeros(len(rays), np.int64), hits
    if debug:
        missed = hits < desc.maxBounce
    else:
        rad2, after2 = orc.calc_color(tris, spheres, bright_sky(scene), desc.trianglesOnly, rays, state, mb, False)
        assert np.array_equal(after, after2)
        missed = (rad.view(np.uint32) != rad2.view(np.uint32)).any(1)
    return rad, after, hits + missed, hits


def reference_pass(tris, spheres, scene, cam, desc, first, count, state=None, cache=None):
    """(accum float32 [rows, W, 3], rng uint32 [rows, W], colors uint8 [rows, W, 3], segments) after samples
    [first, first + count) from `state` = (accum, rng) of the first `first` samples (None with first == 0)."""
    assert (state is None) == (first == 0) and count > 0 and first + count <= desc.spp
    L = _launch(desc)
    shape = (L.rows(), desc.width)
    rays = launch_rays(cam, L)
    if state is None:
        acc, rng = np.zeros((len(rays), 3), F), seeds(desc)
    else:
        acc, rng = np.array(state[0], F).reshape(-1, 3), np.array(state[1], np.uint32).reshape(-1)
    w = F(1.0 / np.float64(desc.spp))  # (float)(1. / accumulationCount), main.c:99
    segments = 0
    with np.errstate(all="ignore"):
        for _ in range(count):
            rad, rng, calls, _ = sample(tris, spheres, scene, desc, rays, rng, cache)
            acc = (acc + (rad * w).astype(F)).astype(F)
            segments += int(calls.sum())
    return acc.reshape(*shape, 3), rng.reshape(shape), to_color(acc).reshape(*shape, 3), segments


def hits_per_sample(tris, spheres, scene, cam, desc, cache=None):
    """int64 [spp, pixels]: the hits of every sample of the frame (what moves a pixel's state, 7 draws each)."""
    rays, rng, out = launch_rays(cam, _launch(desc)), seeds(desc), []
    for _ in range(desc.spp):
        _, rng, _, h = sample(tris, spheres, scene, desc, rays, rng, cache)
        out.append(h)
    return np.stack(out)


def chain(tris, spheres, scene, cam, desc, split, cache=None):
    """reference_pass over the passes of `split` (sample counts summing to desc.spp): the list of (samples done, accum,
    rng, colors, segments of the pass)."""
    assert sum(split) == desc.spp
    out, done, state = [], 0, None
    for count in split:
        acc, rng, col, seg = reference_pass(tris, spheres, scene, cam, desc, done, count, state, cache)
        done, state = done + count, (acc, rng)
        out.append((done, acc, rng, col, seg))
    return out


# ---- the scenes of tests/test_progressive_reference.py and tests/test_gpu_progressive.py (committed fixtures) ----------
SCENE_NAMES = ("ultracomplex", "fsuzane", "default", "open5", "chunks")


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(triangles, spheres or None, Scene, camera, trianglesOnly): ultracomplex and fsuzane (many hits per sample), the
    reference's default box with its sphere (closed: the one-lane-per-pixel kernel), ultracomplex with the five open
    spheres of tests/sphere_scenes.py (the sphere split) and the two-chunk scene of tests/adversarial_scenes.py."""
    import raytracingc_amd as rt
    from adversarial_scenes import SCENES
    from conftest import load_tris, scene_spheres
    from sphere_scenes import open5

    scene, cam = rt.default_scene(), rt.camera_basis()
    if name in ("ultracomplex", "fsuzane"):
        return load_tris(name)[0], None, scene, cam, 1
    if name == "default":
        return load_tris("default")[0], scene_spheres("default"), scene, cam, 0
    if name == "open5":
        return load_tris("ultracomplex")[0], open5(), scene, cam, 0
    if name == "chunks":
        return SCENES["chunks"][0], None, scene, SCENES["chunks"][1], 1
    if name == "chunks_open5":  # (not in SCENE_NAMES: two chunks AND spheres, for the sphere split's passes alone)
        return SCENES["chunks"][0], open5(), scene, SCENES["chunks"][1], 0
    raise KeyError(name)
