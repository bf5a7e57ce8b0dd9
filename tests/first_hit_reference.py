"""What rtc_render_first_hit_async must write (include/rtc.h), from the CPU oracle alone: the launch's primary
rays (tests/primary_rays.launch_rays, main.c:88-94) through oracle.binding.calc_path with max_bounce = 1, whose first call
is calculateRayCollision(ray, trianglesOnly) (raytracing.c:216-240).  Shared by tests/test_gpu_first_hit.py (the GPU's
buffers, bit for bit) and tests/test_first_hit_reference.py (the premises of those cases, without a GPU); each case's
expectation is computed once and is read-only."""
from __future__ import annotations

import functools

import numpy as np

import adversarial_scenes as adv
import oracle.binding as orc
import raytracingc_amd as rt
import sphere_scenes
from conftest import load_tris, scene_spheres
from primary_rays import launch_rays
from raytracingc_amd._abi import SPHERE_DT, TRIANGLE_DT

NAMES = ("prim", "depth", "normal", "albedo")
SHAPES = ((33, 17), (64, 40))  # partial tiles on both edges; more than one workgroup block each way
LARGE = (1024, 400)            # 409,600 pixels: the superblock level of the cull runs (rtc_plan.h kSuperCullPixels)
GOLDEN = ("simplest", "cube", "default_spheres", "default", "suze")
# The default scene is a closed box around its golden camera (main.c:114-116): every primary ray hits, so those two cases
# have hits on triangles and on the sphere but no miss.  The same scene from outside the box has both.
CLOSED = ("default_spheres", "default")
OUTSIDE = ("default_spheres_outside", "default_outside")
OUTSIDE_CAMERA = ((-11.0, -3.5, -11.0), (0.9, -1.2, 1.0), 1.0)
ADVERSARIAL = ("ties_axis", "ties_tilted", "ties_rotated", "slivers", "near_eps", "origin_in_plane", "bad_normals",
               "nonfinite")
SPHERE_CASES = ("tie_scene", "open33", "closing_sphere")


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(triangles or None, spheres or None, trianglesOnly, camera) of a case."""
    if name in adv.SCENES:
        tris, cam, _ = adv.SCENES[name]
        return tris, None, 1, cam
    if name == "tie_scene":
        t, s = sphere_scenes.tie_scene()
        return t, s, 0, adv.camera()
    if name == "open33":  # more than the split launch's 32 spheres
        return load_tris("ultracomplex")[0], sphere_scenes.open5_padded(33), 0, rt.camera_basis()
    if name == "closing_sphere":  # no triangle at all; the camera inside the sphere: the root -b + delta, no miss
        return None, sphere_scenes.closing_sphere(), 0, rt.camera_basis()
    if name.startswith("default"):  # the default scene as the reference renders it: its 14 triangles and its sphere
        cam = rt.camera_basis(*OUTSIDE_CAMERA) if name.endswith("_outside") else rt.camera_basis()
        return load_tris("default")[0], scene_spheres("default"), int("spheres" not in name), cam
    return load_tris(name)[0], None, 1, rt.camera_basis()


def config(name, shape, **kw):
    return rt.RenderConfig(shape[0], shape[1], 0, 0, bool(geometry(name)[2]), **kw)


def expected_for(tris, spheres, tonly, cam, cfg):
    """{prim int32 [rows, W], depth float32 [rows, W], normal, albedo float32 [rows, W, 3]} of the launch cfg."""
    rays = launch_rays(cam, cfg)
    n = len(rays)
    tris = np.zeros(0, TRIANGLE_DT) if tris is None else np.ascontiguousarray(tris, TRIANGLE_DT)
    spheres = np.zeros(0, SPHERE_DT) if spheres is None else np.ascontiguousarray(spheres, SPHERE_DT)
    _, _, calls, ncalls = orc.calc_path(tris, spheres, rt.default_scene(), int(tonly), rays, np.zeros(n, np.uint32),
                                        np.ones(n, np.int32))
    assert (ncalls == 1).all()
    winner, dst = calls[:, 0]["winner"].astype(np.int32), calls[:, 0]["dst"].astype(np.float32)
    normal, albedo = np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32)  # bit patterns: +0 on a miss
    t = winner >= 0
    if t.any():  # the stored normal and the material colour, bit for bit (dwords 9-11 and 12-14 of a Triangle)
        words = tris.view(np.uint32).reshape(len(tris), 17)
        normal[t], albedo[t] = words[winner[t], 9:12], words[winner[t], 12:15]
    s = winner <= -2
    if s.any():  # raySphere's own normal (raytracing.c:181-182); the colour: dwords 4-6 of a Sphere
        which = spheres[-2 - winner[s]]
        hit, sdst, nrm = orc.ray_sphere(rays[s], which)
        assert hit.all() and np.array_equal(sdst.view(np.uint32), dst[s].view(np.uint32))
        normal[s] = nrm.view(np.uint32)
        albedo[s] = spheres.view(np.uint32).reshape(len(spheres), 9)[-2 - winner[s], 4:7]
    rows = cfg.rows()
    out = {"prim": winner.reshape(rows, cfg.width), "depth": dst.reshape(rows, cfg.width),
           "normal": normal.view(np.float32).reshape(rows, cfg.width, 3),
           "albedo": albedo.view(np.float32).reshape(rows, cfg.width, 3)}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, shape, row_start=0, row_stride=1, row_band=0):
    tris, spheres, tonly, cam = geometry(name)
    return expected_for(tris, spheres, tonly, cam, config(name, shape, row_start=row_start, row_stride=row_stride,
                                                          row_band=row_band))


def differing(got, want):
    """{buffer: pixels whose uint32 bit patterns differ} over the buffers of `got`."""
    out = {}
    for k, g in got.items():
        d = np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(want[k]).view(np.uint32)
        out[k] = int((d.any(-1) if d.ndim == 3 else d).sum())
    return out
