"""Moved geometry for the tests of the in-place scene update (tests/test_refit_host.py, tests/test_gpu_scene_update.py;
rtc_scene_update_async has no reference counterpart: main.c:229-243 builds its arrays once).  Deterministic float32
numpy on Triangle[] arrays; the normals and the materials stay as they are (a translation keeps a normal, and the
renderer takes the stored normal as given)."""
from __future__ import annotations

import numpy as np

from raytracingc_amd._abi import TRIANGLE_DT

VERTS = ("posA", "posB", "posC")
SHIFT = (0.4, -0.3, 0.2)


def _moved(tris, fn) -> np.ndarray:
    """A copy of tris with fn(vertex name, xyz float32 [n, 3]) -> float32 [n, 3] applied to every vertex array."""
    out = np.ascontiguousarray(tris, TRIANGLE_DT).copy()
    for v in VERTS:
        p = np.stack([out[v][c] for c in "xyz"], 1).astype(np.float32)
        q = np.asarray(fn(v, p), np.float32)
        for k, c in enumerate("xyz"):
            out[v][c] = q[:, k]
    return out


def shift(tris, scale: float = 1.0) -> np.ndarray:
    """Every third triangle (index 0, 3, 6, ..) translated by scale x (0.4, -0.3, 0.2)."""
    d = np.float32(scale) * np.asarray(SHIFT, np.float32)
    sel = (np.arange(len(tris)) % 3 == 0)[:, None]
    return _moved(tris, lambda v, p: np.where(sel, p + d, p))


def scatter(tris, seed: int = 7) -> np.ndarray:
    """Every triangle translated by its own seeded vector in [-3, 3]^3: the upload's clusters lose their locality (huge
    balls, overlapping chunk balls)."""
    d = np.random.default_rng(seed).uniform(-3.0, 3.0, (len(tris), 3)).astype(np.float32)
    return _moved(tris, lambda v, p: p + d)


def squash(tris, factor: float = 0.25) -> np.ndarray:
    """z scaled by `factor` about the centroid of all vertices: edges, margins and aligned-normal verdicts change (the
    stored normals no longer match the geometric ones)."""
    t = np.ascontiguousarray(tris, TRIANGLE_DT)
    zc = np.float32(np.mean([t[v]["z"].astype(np.float64).mean() for v in VERTS])) if len(t) else np.float32(0)
    f = np.float32(factor)

    def fn(v, p):
        q = p.copy()
        q[:, 2] = zc + (p[:, 2] - zc) * f
        return q

    return _moved(tris, fn)


HELPERS = {"shift": shift, "scatter": scatter, "squash": squash}


def synthetic(n: int, seed: int = 3) -> np.ndarray:
    """n small triangles on a jittered grid in front of the default camera, facing it: scenes of exact sizes (a partial
    last cluster, exactly one chunk, a second chunk of one cluster)."""
    rng = np.random.default_rng(seed + n)
    t = np.zeros(n, TRIANGLE_DT)
    side = int(np.ceil(np.sqrt(max(n, 1))))
    for i in range(n):
        a = np.array([-2.0 + 4.0 * (i % side) / side, -3.0 + 3.0 * (i // side) / side, 1.0 + 0.01 * (i % 7)])
        a = (a + rng.uniform(-0.02, 0.02, 3)).astype(np.float32)
        e1 = np.array([0.3 + 0.1 * rng.random(), 0.02 * rng.random(), 0.05 * rng.random()], np.float32)
        e2 = np.array([0.02 * rng.random(), 0.3 + 0.1 * rng.random(), 0.05 * rng.random()], np.float32)
        nrm = np.cross(e1.astype(np.float64), e2.astype(np.float64))
        nrm /= np.linalg.norm(nrm)
        if nrm[2] > 0:  # towards the camera (it looks along +z from z < 0)
            nrm = -nrm
        t[i]["posA"], t[i]["posB"], t[i]["posC"] = tuple(a), tuple(a + e1), tuple(a + e2)
        t[i]["normal"] = tuple(nrm.astype(np.float32))
        t[i]["mat"]["color"] = (0.3 + 0.7 * rng.random(), 0.3 + 0.7 * rng.random(), 0.3 + 0.7 * rng.random())
        t[i]["mat"]["emissionStrength"] = 0.5 if i % 5 == 0 else 0.0
        t[i]["mat"]["smoothness"] = 0.25 * (i % 4)
    return t
