"""Sphere scenes of the sphere-split tests (tests/test_plan_spheres.py, tests/test_gpu_sphere_split.py) and of
tools/sphere_split_probe.py: Sphere[] arrays (raytracing.h:34-39) beside the golden Triangle[] scenes."""
from __future__ import annotations

import numpy as np

from raytracingc_amd._abi import SPHERE_DT, TRIANGLE_DT


def spheres(rows) -> np.ndarray:
    """Sphere[] from rows of (pos, r, colour, emission, smoothness)."""
    s = np.zeros(len(rows), SPHERE_DT)
    for i, (pos, r, col, em, sm) in enumerate(rows):
        s[i]["pos"] = tuple(pos)
        s[i]["r"] = r
        s[i]["mat"]["color"] = tuple(col)
        s[i]["mat"]["emissionStrength"] = em
        s[i]["mat"]["smoothness"] = sm
    return s


# open5: a mirror ball, a glossy red one, a lamp, a huge ground sphere under the model and one behind the default camera
OPEN5_ROWS = [
    ((1.5, -1.0, 1.5), 0.9, (1.0, 1.0, 1.0), 0.0, 1.0),
    ((-0.5, -0.6, 0.5), 0.5, (1.0, 0.2, 0.2), 0.0, 0.6),
    ((0.5, -2.6, 2.5), 0.6, (1.0, 0.9, 0.7), 4.0, 0.0),
    ((0.0, 40.4, 3.0), 40.0, (0.5, 0.5, 0.5), 0.0, 0.0),
    ((-8.0, -1.5, -8.0), 1.0, (0.0, 1.0, 0.0), 0.0, 0.0),
]


def open5() -> np.ndarray:
    return spheres(OPEN5_ROWS)


# 27 small spheres that pad open5 to exactly 32 (and one more to 33): a row of beads in front of the model, radius 0.08,
# alternating diffuse grey and faint emitters
PAD_ROWS = [((-2.0 + 0.16 * k, -0.3 - 0.05 * (k % 3), -1.0 + 0.1 * (k % 5)), 0.08,
             (0.3 + 0.02 * k, 0.8 - 0.02 * k, 0.5), 0.5 * (k % 2), 0.25 * (k % 4)) for k in range(28)]


def open5_padded(n: int) -> np.ndarray:
    assert 5 <= n <= 5 + len(PAD_ROWS)
    return spheres(OPEN5_ROWS + PAD_ROWS[:n - 5])


def closing_sphere(r: float = 50.0, centre=(-4.75, -1.5, -4.75)) -> np.ndarray:
    """One sphere of radius r around the default camera (and the model): every primary ray hits something, and rays that
    start inside take raySphere's -b + delta root (raytracing.c:174-176)."""
    return spheres([(centre, r, (0.7, 0.7, 0.8), 0.2, 0.1)])


def tie_scene():
    """(triangles, spheres): one emissive green triangle in the plane z = 4 and two identical emissive spheres (red, then
    blue) at (0, 0, 5), r 1: along the centre ray of a camera at the origin looking down +z both the triangle and the
    spheres are at distance exactly 4.0f -- the reference keeps the first sphere (index order, strict <)."""
    t = np.zeros(1, TRIANGLE_DT)
    t[0]["posA"] = (-4.0, -4.0, 4.0)
    t[0]["posB"] = (4.0, -4.0, 4.0)
    t[0]["posC"] = (0.0, 6.0, 4.0)
    t[0]["normal"] = (0.0, 0.0, -1.0)
    t[0]["mat"]["color"] = (0.0, 1.0, 0.0)
    t[0]["mat"]["emissionStrength"] = 1.0
    s = spheres([((0.0, 0.0, 5.0), 1.0, (1.0, 0.0, 0.0), 1.0, 0.0), ((0.0, 0.0, 5.0), 1.0, (0.0, 0.0, 1.0), 1.0, 0.0)])
    return t, s
