"""The ray sets of tests/test_gpu_trace_paths_wave.py (RTC_F_WAVE_PER_RAY) as plain data, shared with
tests/test_trace_paths_wave_reference.py, which shows their premises with the CPU oracle alone.  The scenes are
tests/chain_path_scenes.py's, tests/trace_rays_reference.py's and tests/primary_rays.py's; the expectations are
tests/trace_paths_reference.py's.  Every set is computed once and is read-only; none holds more than 2,560 rays.

The window's edges (a wave evaluates 64 candidate samples, 7 draws apart, and walks them by their hit counts):
  box_mirror / box_gloss   every sample makes exactly maxBounce hits: maxBounce 63 puts the second sample on the last lane,
                           64 exactly at the window's end, 65 and 100 past it (one sample per window, a jump of 7 k > 448);
                           maxBounce 1 and 2 at spp 64, 65, 130: every lane (every second lane) a sample, a last window of
                           one or two
  box_diffuse_T            mixed hit counts (about three per sample), several windows at spp 130, maxBounce 40
  miss rays                h == 0: the sample drew nothing, every remaining sample is the same one"""
from __future__ import annotations

import functools

import numpy as np

import chain_path_scenes as cps
import moving_scenes
import raytracingc_amd as rt
import trace_paths_reference as tp
import trace_rays_reference as tr
from primary_rays import launch_rays
from raytracingc_amd._abi import RAY_DT, SPHERE_DT, TRIANGLE_DT

BOX_SHAPE = (16, 8)
# (scene, spp, maxBounce) on the scene's 16 x 8 primary rays
WINDOW_CASES = tuple((name, 5, mb) for name in ("box_mirror", "box_gloss") for mb in cps.MIRROR_BOUNCES) + \
    tuple(("box_gloss", spp, mb) for mb in (1, 2) for spp in (64, 65, 130)) + (("box_diffuse_T", 130, 40),)
SAMPLE_COUNTS = (1, 2, 3, 5, 63, 64, 65, 130)
MISS_SCENE = "suze"
MISS_SPPS = (1, 2, 130)
ACC0_VALUES = (1e30, float("inf"), float("nan"), -0.0, 0.0)


@functools.lru_cache(maxsize=None)
def frame_rays(name, width, height):
    """The width x height launch's primary rays of a scene of chain_path_scenes (pixel y * width + x)."""
    rays = launch_rays(tp.geometry(name)[3], rt.RenderConfig(width, height, 0, 0, True))
    rays.setflags(write=False)
    return rays


def box_rays(name):
    return frame_rays(name, *BOX_SHAPE)


@functools.lru_cache(maxsize=None)
def window_expected(name, spp, max_bounce):
    tris, spheres, tonly, _ = tp.geometry(name)
    rays = box_rays(name)
    return tp.expected(tris, spheres, rt.default_scene(), tonly, rays, tp.pixel_seeds(len(rays)), spp, max_bounce)


@functools.lru_cache(maxsize=None)
def suze_rays():
    """Every 20th primary ray of suze's 64 x 40 launch with its pixel's seed: hits and misses."""
    rays = tp.camera_rays("suze")[::20]
    seeds = tp.pixel_seeds(tp.SHAPE[0] * tp.SHAPE[1])[::20]
    return rays, seeds


@functools.lru_cache(maxsize=None)
def suze_expected(spp):
    tris, spheres, tonly, _ = tp.geometry("suze")
    rays, seeds = suze_rays()
    return tp.expected(tris, spheres, rt.default_scene(), tonly, rays, seeds, spp, tp.MAX_BOUNCE)


@functools.lru_cache(maxsize=None)
def miss_rays():
    """65 rays (a workgroup's four waves sixteen times, and one) that start behind suze's camera and point away from the
    mesh, over and under the horizon and across the sun: they hit nothing."""
    rays = np.zeros(65, RAY_DT)
    k = np.arange(65)
    rays["pos"]["z"] = -50.0
    rays["dir"]["x"] = ((k % 13) - 6) * np.float32(0.25)
    rays["dir"]["y"] = ((k // 13) - 2) * np.float32(0.375)
    rays["dir"]["z"] = -1.0
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def miss_acc0():
    """float32 [65, 3]: row i holds ACC0_VALUES[i % 5] three times."""
    a = np.repeat(np.array(ACC0_VALUES, np.float32)[np.arange(65) % 5][:, None], 3, 1)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def miss_expected(spp, first=0):
    tris, spheres, tonly, _ = tp.geometry(MISS_SCENE)
    rays = miss_rays()
    return tp.expected(tris, spheres, rt.default_scene(), tonly, rays, tp.hash_seeds(len(rays)), spp, tp.MAX_BOUNCE, first,
                       None, miss_acc0() if first else None)


def pass_frame(frame):
    """(scene, rays, seeds, maxBounce) of one of chain_path_scenes.PASS_FRAMES."""
    name, w, h, mb = cps.PASS_FRAMES[frame]
    rays = frame_rays(name, w, h)
    return name, rays, tp.pixel_seeds(len(rays)), mb


@functools.lru_cache(maxsize=None)
def pass_expected(frame):
    name, rays, seeds, mb = pass_frame(frame)
    tris, spheres, tonly, _ = tp.geometry(name)
    return tp.expected(tris, spheres, rt.default_scene(), tonly, rays, seeds, sum(cps.PASS_SPLIT), mb)


# trace_rays_reference's sets, spp 3 with hashed seeds: (kind, scene, scale)
CALLER_SETS = (("replay", "chunks", None), ("replay", "slivers", None), ("replay", "mixed_scale", None),
               ("scaled", "chunks", 3.0), ("scaled", "chunks", 1e4))
RAY_COUNTS = (1, 3, 4, 5)  # a workgroup takes four rays
NO_BOUNCE = (0, -5)
UPDATE_MOVE = "shift"


def count_rays(n):
    """The first n bounce rays of chunks, spp 3."""
    return tr.replay("chunks")[:n], tp.hash_seeds(max(RAY_COUNTS))[:n]


def edge_rays():
    """70 bounce rays of chunks (the optional outputs and maxBounce <= 0), spp 3."""
    return tr.replay("chunks")[:70], tp.hash_seeds(70)


@functools.lru_cache(maxsize=None)
def update_rays():
    """Bounce rays and camera rays of chunks, before and after a step of tests/moving_scenes.py, spp 2."""
    rays = np.concatenate([tr.replay("chunks")[:500], tp.camera_rays("chunks")[::5]])
    rays.setflags(write=False)
    return rays, tp.hash_seeds(len(rays))


def host_rays():
    """700 bounce rays of the default scene with its sphere, spp 5: the host entry's."""
    rays = tr.replay("default")[:700]
    return rays, tp.hash_seeds(len(rays))


def records(tris, spheres):
    """(TRIANGLE_DT [], SPHERE_DT []) for oracle.binding.calc_path: None becomes an empty array."""
    return (np.zeros(0, TRIANGLE_DT) if tris is None else np.ascontiguousarray(tris, TRIANGLE_DT),
            np.zeros(0, SPHERE_DT) if spheres is None else np.ascontiguousarray(spheres, SPHERE_DT))


def all_sets():
    """Every set tests/test_gpu_trace_paths_wave.py runs, for the premise test: (label, triangles, spheres, trianglesOnly,
    rays, seeds, maxBounce, the largest spp the set is run at).  Sets that share rays, seeds, scene and maxBounce and
    differ in spp alone are one entry: a chain's first samples do not depend on how many follow."""
    out = []

    def add(label, name, rays, seeds, max_bounce, spp, tonly=None, tris=None):
        g = tp.geometry(name)
        out.append((label, g[0] if tris is None else tris, g[1], g[2] if tonly is None else tonly, rays, seeds, max_bounce, spp))

    for n in tp.CAMERA_CASES:
        add(f"camera {n}", n, tp.camera_rays(n), tp.pixel_seeds(tp.SHAPE[0] * tp.SHAPE[1]), tp.MAX_BOUNCE, tp.SPP)
    for n, mb in sorted({(n, mb) for n, _, mb in WINDOW_CASES}):
        spp = max(s for m, s, b in WINDOW_CASES if (m, b) == (n, mb))
        add(f"window {n} mb {mb}", n, box_rays(n), tp.pixel_seeds(len(box_rays(n))), mb, spp)
    add("suze[::20]", "suze", *suze_rays(), tp.MAX_BOUNCE, max(SAMPLE_COUNTS))
    add("miss", MISS_SCENE, miss_rays(), tp.hash_seeds(len(miss_rays())), tp.MAX_BOUNCE, max(MISS_SPPS))
    for kind, name, scale in CALLER_SETS:
        rays = tr.case_rays(kind, name, scale)
        add(f"{kind} {name} {scale}", name, rays, tp.hash_seeds(len(rays)), tp.MAX_BOUNCE, 3)
    for tonly in (0, 1):
        rays = tr.odd()[0]
        add(f"odd tonly {tonly}", "default", rays, tp.hash_seeds(len(rays)), tp.MAX_BOUNCE, 3, tonly)
    for frame in sorted(cps.PASS_FRAMES):
        name, rays, seeds, mb = pass_frame(frame)
        add(f"pass {frame}", name, rays, seeds, mb, sum(cps.PASS_SPLIT))
    for n in RAY_COUNTS:
        add(f"count {n}", "chunks", *count_rays(n), tp.MAX_BOUNCE, 3)
    add("edge", "chunks", *edge_rays(), tp.MAX_BOUNCE, 3)
    for mb in NO_BOUNCE:
        add(f"edge mb {mb}", "chunks", *edge_rays(), mb, 3)
    add("update before", "chunks", *update_rays(), tp.MAX_BOUNCE, 2)
    add("update after", "chunks", *update_rays(), tp.MAX_BOUNCE, 2,
        tris=moving_scenes.HELPERS[UPDATE_MOVE](tp.geometry("chunks")[0]))
    add("host", "default", *host_rays(), tp.MAX_BOUNCE, 5)
    return out
