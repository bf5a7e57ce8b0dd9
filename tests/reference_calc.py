"""The inputs of tests/golden/kat_ref_<family>.npz, stated once: per family the scenes whose calcColor (raytracing.c:262-296)
and calcDebugColor (:242-260) the reference itself computed (oracle/ref_unity.c, --kat-calc-raw: raw Triangle[] and Sphere[]
records, so non-finite values and any number of spheres pass) -- for the generator (tests/golden/make_golden.py), for
tests/test_reference_families.py (the CPU oracle against the fixture) and for tests/test_gpu_reference_calc.py (the kernels
against the fixture).  The fixtures hold no geometry and no rays, only the sha256 of the bytes the reference was given:
cases() rebuilds them and the tests check the hashes first.

A case is one scene with a frame shape: its rays are primary_rays.launch_rays(camera, RenderConfig(width, height, ...)) at
a fixed subset of the frame's pixels and its seeds those pixels' indices x + y * width (main.c:95), so a record is what a
render of that frame at one sample per pixel computes for its pixel.  Everything runs under the reference's default sky
(rt.default_scene()), whatever Scene a family's own GPU test renders with.

  adversarial  every entry of adversarial_scenes.SCENES, 48 x 40 (tests/test_gpu_adversarial_frames.py), maxBounce 10
  boxes        every frame of chain_path_scenes.FRAMES with its own width, height and maxBounce (63, 64, 65, 100 among them)
  materials    every scene of material_scenes.SCENES in its own frame's shape, and the three sphere scenes (SPHERE_FRAME)
  spheres      the scenes of tests/test_gpu_sphere_split.py (_geometry) in the shapes of its CASES, open5 with trianglesOnly
               1 as well, and the tie scene at 64 x 64 too, whole and without its triangle: in the whole scene only the
               centre ray has its tie at the closest distance (elsewhere the triangle lies in front of the two equal
               spheres), without the triangle every ray that meets the spheres has
  populations  nothing at all (trianglesOnly 0 and 1), spheres alone, one triangle

The pixel subset: every pixel while a frame has at most the family's MAX_RECORDS, else every s-th pixel in raster order, s the
smallest of STRIDES that is coprime to the width (so every column occurs) and brings the count within it."""
from __future__ import annotations

import functools
import hashlib
import math
from typing import NamedTuple

import numpy as np

import raytracingc_amd as rt
from primary_rays import launch_rays
from raytracingc_amd._abi import SPHERE_DT, TRIANGLE_DT

FAMILIES = ("adversarial", "boxes", "materials", "spheres", "populations")
DEBUG_FAMILIES = ("adversarial", "spheres")  # calcDebugColor as well
MAX_RECORDS = {"adversarial": 400, "boxes": 480, "materials": 480, "spheres": 800, "populations": 600}
STRIDES = (1, 5, 7, 11, 13, 17, 19, 23, 29, 31)
ADVERSARIAL_SHAPE = (48, 40)  # tests/test_gpu_adversarial_frames.py SHAPES["48x40x6"]
ADVERSARIAL_MAX_BOUNCE = 10
TIE_WIDE_SHAPE = (64, 64)


class Case(NamedTuple):
    name: str
    tris: np.ndarray       # TRIANGLE_DT [T], may be empty
    spheres: np.ndarray    # SPHERE_DT [S], may be empty
    triangles_only: int
    camera: object         # RtcCamera
    width: int
    height: int
    max_bounce: int
    pixels: np.ndarray     # int64, indices x + y * width in increasing order


def pixel_subset(width, height, limit, keep=None):
    """`keep`: a pixel the subset must hold (the stride's phase is chosen for it)."""
    n = width * height
    for s in STRIDES:
        if math.gcd(s, width) == 1 and (n + s - 1) // s <= limit:
            return np.arange(0 if keep is None else keep % s, n, s, dtype=np.int64)
    raise ValueError(f"{width} x {height}: no stride of STRIDES brings the frame within {limit} records")


def _case(family, name, tris, spheres, tonly, cam, width, height, max_bounce, keep=None):
    tris = np.zeros(0, TRIANGLE_DT) if tris is None else np.ascontiguousarray(tris, TRIANGLE_DT)
    spheres = np.zeros(0, SPHERE_DT) if spheres is None else np.ascontiguousarray(spheres, SPHERE_DT)
    px = pixel_subset(width, height, MAX_RECORDS[family], keep)
    px.setflags(write=False)
    return Case(name, tris, spheres, int(tonly), cam, int(width), int(height), int(max_bounce), px)


@functools.lru_cache(maxsize=None)
def cases(family):
    """The family's cases, in the fixture's order."""
    out = []
    if family == "adversarial":
        from adversarial_scenes import SCENES

        for name, (tris, cam, _) in SCENES.items():
            out.append(_case(family, name, tris, None, 1, cam, *ADVERSARIAL_SHAPE, ADVERSARIAL_MAX_BOUNCE))
    elif family == "boxes":
        from chain_path_scenes import FRAMES, SCENES

        for frame, (scene, w, h, _, mb) in FRAMES.items():
            tris, cam, _ = SCENES[scene]
            out.append(_case(family, frame, tris, None, 1, cam, w, h, mb))
    elif family == "materials":
        import material_scenes as ms

        for name, (tris, cam, _) in ms.SCENES.items():
            _, w, h, _, mb = ms.FRAMES[name]  # (every scene has a frame of its own name)
            out.append(_case(family, name, tris, None, 1, cam, w, h, mb))
        for name in ms.SPHERE_NAMES:
            tris, sph, cam, _ = ms.sphere_scene(name)
            w, h, _, mb = ms.SPHERE_FRAME
            out.append(_case(family, name, tris, sph, 0, cam, w, h, mb))
    elif family == "spheres":
        import test_gpu_sphere_split as split

        seen = set()
        for name, w, h, _, mb in split.CASES:
            if name in seen:  # (`default` has a second, larger shape: the first one)
                continue
            seen.add(name)
            tris, sph, _, cam = split._geometry(name)
            out.append(_case(family, name, tris, sph, 0, cam, w, h, mb))
            if name == "open5":
                out.append(_case(family, "open5_triangles_only", tris, sph, 1, cam, w, h, mb))
            if name == "tie":  # (the centre ray, where the triangle and both spheres are at 4.0f, is kept)
                w2, h2 = TIE_WIDE_SHAPE
                out.append(_case(family, "tie_wide", tris, sph, 0, cam, w2, h2, mb, keep=w2 // 2 + h2 // 2 * w2))
                out.append(_case(family, "tie_wide_spheres", None, sph, 0, cam, w2, h2, mb))
    elif family == "populations":
        from adversarial_scenes import SCENES
        from sphere_scenes import open5_padded

        cam = rt.camera_basis()
        out.append(_case(family, "empty", None, None, 0, cam, 12, 10, 10))
        out.append(_case(family, "empty_triangles_only", None, None, 1, cam, 12, 10, 10))
        out.append(_case(family, "spheres_alone", None, open5_padded(12), 0, cam, 30, 20, 10))
        # counts_1's one triangle (corners (-2.4, -2, 4), (-1.6, -2, 4.375), (-1.6, -1.3, 4)) covers a pixel or two of a
        # small frame from its own camera: a camera looking at it, fov 10, sees it over a quarter of an odd-sized frame
        tris = SCENES["counts_1"][0]
        out.append(_case(family, "counts_1", tris, None, 1, rt.camera_basis((0.0, 0.0, 0.0), (-1.9, -1.75, 4.1), 10.0),
                         33, 17, 10))
    else:
        raise KeyError(family)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


EMPTY_CASES = ("empty", "empty_triangles_only")  # the only cases without a hit


def config(case, **kw):
    """The RenderConfig of the case's frame at one sample per pixel."""
    return rt.RenderConfig(case.width, case.height, 1, case.max_bounce, bool(case.triangles_only), **kw)


def inputs(case):
    """(Ray[] as RAY_DT, seeds uint32) of the case's records."""
    rays = np.ascontiguousarray(launch_rays(case.camera, config(case))[case.pixels])
    return rays, case.pixels.astype(np.uint32)


def sha256(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def input_hashes(case, rays):
    """What the fixture stores in place of the inputs: the sha256 of the Triangle[], Sphere[] and Ray[] bytes."""
    return sha256(case.tris), sha256(case.spheres), sha256(rays)


class Fixture(NamedTuple):
    """One case's part of kat_ref_<family>.npz."""
    sha_tris: str
    sha_spheres: str
    sha_rays: str
    pixels: np.ndarray
    max_bounce: int
    color: np.ndarray            # float32 [n, 3]
    seed_after: np.ndarray       # uint32 [n]
    debug_color: np.ndarray      # or None
    debug_seed_after: np.ndarray


@functools.lru_cache(maxsize=None)
def fixture(family):
    """{case name: Fixture} of the committed file (read-only arrays).  The file holds the cases one after another: names,
    counts (records per case) and the per-case hashes and maxBounce, then the records' arrays concatenated."""
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"kat_ref_{family}.npz")
    out = {}
    with np.load(path) as k:
        ends = np.cumsum(k["counts"])
        for i, name in enumerate(k["names"]):
            m = slice(int(ends[i] - k["counts"][i]), int(ends[i]))
            part = [np.array(k[key][m]) for key in ("pixels", "color", "seed_after")]
            part += [np.array(k[key][m]) if key in k.files else None for key in ("debug_color", "debug_seed_after")]
            for a in part:
                if a is not None:
                    a.setflags(write=False)
            out[str(name)] = Fixture(str(k["sha_tris"][i]), str(k["sha_spheres"][i]), str(k["sha_rays"][i]),
                                     part[0].astype(np.int64), int(k["max_bounce"][i]), *part[1:])
    return out


def checked_inputs(family, case):
    """(rays, seeds, Fixture) of a case after the check that comes first: the rebuilt inputs are the ones the reference was
    given.  A mismatch fails: the scenes changed and the fixture must be made again."""
    fx = fixture(family).get(case.name)
    hint = f"{family}/{case.name}: regenerate tests/golden/kat_ref_{family}.npz (make ref && python tests/golden/make_golden.py)"
    assert fx is not None, f"no such case in the fixture; {hint}"
    rays, seeds = inputs(case)
    assert np.array_equal(fx.pixels, case.pixels) and fx.max_bounce == case.max_bounce, f"pixels or maxBounce differ; {hint}"
    assert (fx.sha_tris, fx.sha_spheres, fx.sha_rays) == input_hashes(case, rays), f"the inputs' hashes differ; {hint}"
    return rays, seeds, fx


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing(got, want):
    """Records whose float32 bit patterns differ; where the reference has a NaN, any NaN is accepted (the project's
    standing exception: a NaN's sign and payload differ between x86 and gfx950), a number in its place is not."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    return int(d.reshape(len(d), -1).any(-1).sum())
