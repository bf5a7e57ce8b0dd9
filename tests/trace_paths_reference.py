"""What rtc_trace_paths_async must write (include/rtc.h), from the CPU oracle alone: main.c:95-100 with the ray
given -- per sample one oracle.binding.calc_path call (calcColor, raytracing.c:262-296, with its calls counted) with the
seed threaded through, and acc = acc + colour * (float)(1. / spp) as two float32 operations -- and the ray sets of
tests/test_gpu_trace_paths.py (the GPU's radiance and seeds, bit for bit; the segment count, exactly) and
tests/test_trace_paths_reference.py (the helper against the oracle's own render loop, and the sets' premises, without a
GPU).  The ray sets are tests/trace_rays_reference.py's: primary, replay, scaled, odd and the EXTRA scenes.  Every set and
every expectation is computed once and is read-only.

Seeds: a camera ray's is its pixel's, x + y * width (main.c:95) -- the index of the ray in the 64 x 40 launch; every other
ray's is a fixed integer hash of its index (hash_seeds)."""
from __future__ import annotations

import functools

import numpy as np

import material_scenes as ms
import oracle.binding as orc
import raytracingc_amd as rt
import trace_rays_reference as tr
from raytracingc_amd._abi import RAY_DT, SPHERE_DT, TRIANGLE_DT

SHAPE = tr.SHAPE
SPP, MAX_BOUNCE = 5, 10
# the camera cases of tests/test_gpu_trace_paths.py; the first four are tied to oracle.render on the CPU as well
RENDER_CASES = ("suze", "chunks", "default", "box_mirror")
CAMERA_CASES = ("suze", "fsuzane", "chunks", "layers_33", "default", "box_mirror", "spheres_nonfinite", "cbox_nonfinite")
REPLAY_CASES = ("chunks", "slivers", "mixed_scale", "default")


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(triangles or None, spheres or None, trianglesOnly, camera) of a case: trace_rays_reference's, and two scenes of
    tests/material_scenes.py whose accumulators hold inf and NaN."""
    if name == "spheres_nonfinite":
        tris, sph, cam, _ = ms.sphere_scene(name)
        return tris, sph, 0, cam
    if name in ms.SCENES:
        tris, cam, _ = ms.SCENES[name]
        return tris, None, 1, cam
    return tr.geometry(name)


def _records(tris, spheres):
    tris = np.zeros(0, TRIANGLE_DT) if tris is None else np.ascontiguousarray(tris, TRIANGLE_DT)
    spheres = np.zeros(0, SPHERE_DT) if spheres is None else np.ascontiguousarray(spheres, SPHERE_DT)
    return tris, spheres


def hash_seeds(n):
    """uint32 [n]: a fixed integer hash of the ray index (two rounds of multiply and xor-shift: neighbouring rays get
    unrelated RNG chains)."""
    x = np.arange(n, dtype=np.uint64)
    x = (x * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C15)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    out = x.astype(np.uint32)
    out.setflags(write=False)
    return out


def pixel_seeds(n):
    """x + y * width for the rays of a whole launch in raster order (main.c:95)."""
    out = np.arange(n, dtype=np.uint32)
    out.setflags(write=False)
    return out


def expected(tris, spheres, scene, tonly, rays, seeds, spp, max_bounce, first=0, count=None, acc0=None):
    """(radiance float32 [n, 3], seeds_out uint32 [n], segments): samples [first, first + count) of spp (count None: the
    rest) for every ray, the accumulator starting at +0 (first == 0) or at acc0, the RNG state at `seeds`."""
    rays = np.ascontiguousarray(rays, RAY_DT)
    n = len(rays)
    tris, spheres = _records(tris, spheres)
    count = spp - first if count is None else count
    assert 0 <= first and 0 < count <= spp - first
    state = np.array(seeds, np.uint32).reshape(n)
    acc = np.zeros((n, 3), np.float32) if first == 0 else np.array(acc0, np.float32).reshape(n, 3)
    weight = np.float32(1.0 / spp)
    bounces = np.full(n, max_bounce, np.int32)
    segments = 0
    with np.errstate(all="ignore"):
        for _ in range(count):
            colour, state, _, ncalls = orc.calc_path(tris, spheres, scene, int(tonly), rays, state, bounces)
            term = colour * weight
            acc = acc + term
            segments += int(ncalls.sum())
    assert acc.dtype == np.float32 and state.dtype == np.uint32
    acc.setflags(write=False)
    state.setflags(write=False)
    return acc, state, segments


@functools.lru_cache(maxsize=None)
def camera_expected(name, spp=SPP, max_bounce=MAX_BOUNCE):
    """expected() of the case's 64 x 40 primary rays with the pixels' seeds under the default scene."""
    tris, spheres, tonly, _ = geometry(name)
    rays = camera_rays(name)
    return expected(tris, spheres, rt.default_scene(), tonly, rays, pixel_seeds(len(rays)), spp, max_bounce)


@functools.lru_cache(maxsize=None)
def camera_rays(name):
    if name in tr.REPLAY or name in tr.EXTRA:
        return tr.primary(name)
    from primary_rays import launch_rays

    tonly, cam = geometry(name)[2:]
    rays = launch_rays(cam, rt.RenderConfig(SHAPE[0], SHAPE[1], 0, 0, bool(tonly)))
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def set_expected(kind, name, scale=None, spp=3, max_bounce=MAX_BOUNCE, triangles_only=None):
    """expected() of one of trace_rays_reference's sets (replay / scaled / odd / extra) with hashed seeds under the default
    scene; odd: against the default scene's geometry."""
    tris, spheres, tonly, _ = geometry("default" if kind == "odd" else name)
    rays = tr.case_rays(kind, name, scale)
    tonly = tonly if triangles_only is None else triangles_only
    return expected(tris, spheres, rt.default_scene(), tonly, rays, hash_seeds(len(rays)), spp, max_bounce)


def differing(got, want):
    """The number of rays (rows) whose uint32 bit patterns differ, under the project's standing exception
    (tests/test_gpu_materials.py): where the reference gives a NaN, any NaN is accepted."""
    g = np.ascontiguousarray(got).view(np.uint32)
    w = np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (g.shape, w.shape)
    d = g != w
    if np.asarray(want).dtype == np.float32:
        d &= ~(np.isnan(np.ascontiguousarray(got).view(np.float32)) & np.isnan(np.ascontiguousarray(want).view(np.float32)))
    return int((d.any(-1) if d.ndim == 2 else d).sum())
