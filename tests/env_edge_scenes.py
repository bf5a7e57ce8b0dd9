"""Environments at the edges of what the sky kernel's shortcuts accept, as whole small frames (tests/test_gpu_env_frames.py),
and the float32 restatements of main.c those tests and tests/test_gpu_sphere_split.py classify pixels with.

Boundary frames: the camera looks along a direction v with focus * log2(dot(v, sun)) at the scene's sun-skip boundary
(rtc_device.h env_vanish_limit), so the frame holds pixels on both sides of it.  Edge-parameter frames: the special values
of getEnvironmentLight's powf (raytracing.c:153-158) -- focus 0, negative, tiny; intensity negative, -0, +-inf, NaN, huge;
colour components +0 and -0 -- with one scene for the whole launch, looking along the horizon and across the sun's
terminator (dot(dir, sun) = 0)."""
from __future__ import annotations

import math

import numpy as np

import raytracingc_amd as rt
from raytracingc_amd._abi import RAY_DT, SCENE_DT, TRIANGLE_DT, Scene

W, H, SPP, MAX_BOUNCE = 96, 54, 3, 10
SUN = (0.3, -1.0, 0.2)
M60 = 2.0 ** -60 * (1.5 + 2.0 ** -23)  # an odd mantissa: e + sv rounds away from e when sv is half its spacing
M30 = 2.0 ** -30 * (1.25 + 2.0 ** -23)


def primary_rays(cam, width, height):
    """main.c:88-94 in float32 (the renderer's primary_dir; used only to classify pixels)."""
    f = np.float32
    v = lambda a: np.array([a.x, a.y, a.z], f)  # noqa: E731
    xs, ys = np.meshgrid(np.arange(width), np.arange(height))
    dx = ((xs - width // 2).astype(f) / f(height // 2))[..., None]
    dy = ((ys - height // 2).astype(f) / f(height // 2))[..., None]
    d = (v(cam.ex) * dx + v(cam.ey) * dy + v(cam.ez) * f(cam.fov)).astype(f)
    d = d * (f(1) / np.sqrt((d * d).sum(-1, dtype=f)))[..., None]
    rays = np.zeros(width * height, RAY_DT)
    for k, c in enumerate("xyz"):
        rays["pos"][c] = v(cam.origin)[k]
        rays["dir"][c] = d[..., k].reshape(-1)
    return rays


def pixel_sum(e, spp):
    """main.c:97-99 on a camera ray that misses, in float32: the sample is calcColor's light = 0 + environment * (1, 1, 1)
    (raytracing.c:289-291); the pixel's sum starts at +0 and takes sum + sample * (1 / spp) per sample."""
    f = np.float32
    with np.errstate(all="ignore"):
        term = ((f(0) + e.astype(f)).astype(f) * f(1.0 / spp)).astype(f)
        acc = np.zeros_like(term)
        for _ in range(spp):
            acc = (acc + term).astype(f)
    return acc


def scene_record(sun, horizon, zenith, ground, focus, intensity):
    """A Scene (raytracing.h:7-11) as a SCENE_DT record, the sun normalised."""
    s = np.zeros(1, SCENE_DT)
    sun = np.asarray(sun, np.float64)
    sun = (sun / np.linalg.norm(sun)).astype(np.float32)
    for k, v in (("normalizedSunDirection", sun), ("skyColorHorizon", horizon), ("skyColorZenith", zenith),
                 ("groundColor", ground)):
        s[k]["x"], s[k]["y"], s[k]["z"] = v
    s["sunFocus"], s["sunIntensity"] = focus, intensity
    return s[0]


def scene_struct(rec) -> Scene:
    return Scene.from_buffer_copy(np.asarray(rec, SCENE_DT).tobytes())


def _sun(rec):
    return np.array([rec["normalizedSunDirection"][c] for c in "xyz"], np.float64)


def camera_towards(v, fov):
    """A camera at the origin looking along v (main.c:252-255)."""
    return rt.camera_basis((0.0, 0.0, 0.0), tuple(float(c) for c in v), fov)


def camera_at_cosine(rec, cosine, fov):
    """A camera at the origin looking along a direction v with dot(v, sun) = cosine, on the sun's side of the horizon
    (v.y < 0, raytracing.c:156), in the vertical plane of the sun: the camera's ex (main.c:253, horizontal) is then
    perpendicular to the sun, so the lines of constant dot(dir, sun) run along the frame's rows through its centre -- as
    the sky kernel's waves do (64 pixels of a row), which skip the sun's powf only where every lane may."""
    s = _sun(rec)
    up = np.array((0.0, -1.0, 0.0))
    p = up - (up @ s) * s
    p /= np.linalg.norm(p)
    v = cosine * s + math.sqrt(1.0 - cosine * cosine) * p
    assert v[1] < 0
    return camera_towards(v, fov)


def corner_triangle(cam, width=W, height=H):
    """One small diffuse triangle over the pixels (2, 2), (10, 2), (2, 8) of the frame, facing the camera, about 10 units
    away: the split launch gets a geometry list, and nearly every pixel is left to the sky kernel."""
    ex, ey, ez = (np.array([a.x, a.y, a.z], np.float64) for a in (cam.ex, cam.ey, cam.ez))

    def at(px, py):
        d = ex * ((px - width // 2) / (height // 2)) + ey * ((py - height // 2) / (height // 2)) + ez * cam.fov
        return tuple(10.0 * d / np.linalg.norm(d))

    t = np.zeros(1, TRIANGLE_DT)
    t[0]["posA"], t[0]["posB"], t[0]["posC"] = at(2, 2), at(10, 2), at(2, 8)
    t[0]["normal"] = tuple(-ez)
    t[0]["mat"]["color"] = (0.8, 0.7, 0.6)
    t[0]["mat"]["emissionStrength"] = 0.0
    t[0]["mat"]["smoothness"] = 0.25
    return t


def skip_line(rec):
    """log2(H / intensity) - 1e-5 for the scene (H = 2^(floor(log2(m (1 - 2^-20))) - 24), m the smallest colour component):
    the line round 6 drew for every accepted scene; env_vanish_limit keeps it where log2(H / intensity) >= -132."""
    cols = [float(rec[k][c]) for k in ("groundColor", "skyColorHorizon", "skyColorZenith") for c in "xyz"]
    e = math.floor(math.log2(min(cols) * (1 - 2.0 ** -20)))
    return math.log2(2.0 ** (e - 24) / float(rec["sunIntensity"])) - 1e-5


def ylogx_of(rec, rays):
    """focus * log2(x) per ray, x = dot(dir, sun) in float32 as raytracing.c:155 forms it; +inf where sun_vanishes never
    skips (dir.y >= 0, or x not a normal float below 1)."""
    d = np.stack([rays["dir"][c] for c in "xyz"], 1).astype(np.float32)
    sun = _sun(rec).astype(np.float32)
    x = (d[:, 0] * sun[0] + d[:, 1] * sun[1]) + d[:, 2] * sun[2]
    ok = (d[:, 1] < 0) & (x >= 2.0 ** -126) & (x < 1)
    y = np.full(len(x), np.inf)
    y[ok] = float(rec["sunFocus"]) * np.log2(x[ok].astype(np.float64))
    return y


def _uniform(m, focus, intensity):
    return scene_record(SUN, (m, m, m), (m, m, m), (m, m, m), focus, intensity)


def _default_record():
    return np.frombuffer(bytes(rt.default_scene()), SCENE_DT)[0].copy()


def boundary_frames():
    """name -> (scene record, camera).  tie: log2(H / intensity) = -148, where powf's subnormal result makes the sun term
    exactly H on most pixels just below the line (aimed 0.2 below it); i71 / i73: -125 and -127, powf's result at the line
    the last normal floats; default: the headline scene's line (x ~ 0.447)."""
    out = {}
    for name, rec, below, fov in (("tie", _uniform(M60, 250.0, 2.0 ** 64), 0.2, 40.0),
                                  ("i71", _uniform(M30, 22.0, 2.0 ** 71), 0.0, 40.0),
                                  ("i73", _uniform(M30, 22.0, 2.0 ** 73), 0.0, 40.0),
                                  ("default", _default_record(), 0.0, 4.0)):
        cosine = 2.0 ** ((skip_line(rec) + 1e-5 - below) / float(rec["sunFocus"]))
        out[name] = (rec, camera_at_cosine(rec, cosine, fov))
    return out


HORIZON, ZENITH, GROUND = (1.0, 1.0, 1.0), (0.3, 0.9, 0.8), (0.6, 0.6, 0.6)
EDGE_SUN = (1.0, -0.5, 0.2)  # low in the sky: its terminator crosses the horizon at a wide angle in the frame
INF, NAN = math.inf, math.nan
# (focus, intensity, zenith colour): rtc_probe_environment's special values (tests/test_gpu_parity.py kat_env_edge), one
# scene per launch
EDGE_PARAMS = {
    "f0": (0.0, 0.75, ZENITH),
    "fm1_ineg": (-1.0, -0.75, ZENITH),
    "fm3_i1e30": (-3.0, 1e30, ZENITH),
    "fhalf_iinf": (0.5, INF, ZENITH),
    "ftiny_iminf": (1e-30, -INF, ZENITH),
    "f22_inan": (22.0, NAN, ZENITH),
    "fm1_imzero": (-1.0, -0.0, ZENITH),
    "f22_zero_colour": (22.0, 0.75, (0.3, 0.9, 0.0)),
    "f3_imzero_mzero_colour": (3.0, -0.0, (0.3, -0.0, 0.8)),
    "fhalf_i1e30": (0.5, 1e30, ZENITH),
}


def edge_frames():
    """name -> (scene record, camera): the camera looks along the horizon, perpendicular to the sun, fov 1."""
    out = {}
    for name, (focus, intensity, zenith) in EDGE_PARAMS.items():
        rec = scene_record(EDGE_SUN, HORIZON, zenith, GROUND, focus, intensity)
        v = np.cross(_sun(rec), (0.0, 1.0, 0.0))
        out[name] = (rec, camera_towards(v, 1.0))
    return out
