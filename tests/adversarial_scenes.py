"""Geometry at the edges of the culling proofs, as plain data: SCENES maps a name to (Triangle[] as TRIANGLE_DT,
RtcCamera, note).  Everything is written out or built from fixed arithmetic (no random draws).  A note that contains
"filter active" says the primary filter must reject most non-hit (pixel, triangle) pairs there; "sane straddle" that the
scene has hit triangles on both sides of rtc_prep_primary's `sane` switch; "oversized" / "degenerate" / "misaligned" that
some records are ones the cluster and reach proofs do not cover (tests/test_gpu_cluster.py skips its non-vacuity there;
"oversized edges": edges longer than ED_RATIO_EDGE, whose clusters ball_of never culls).

World: the camera basis of main.c:252-255 has up = (0, -1, 0), so +y is down in the image; "floor" triangles lie at
y > 0 with the normal (0, -1, 0).  rayTriangle (raytracing.c:186-214) is two-sided in the winding and one-sided in the
stored normal, so every triangle built here takes a stored normal that faces the camera unless the scene says otherwise.

The counts_* scenes stop at 65 triangles (9 clusters) and `chunks` has 36 clusters: the cluster-count classes between them
(16, 17, 32, 33 clusters) and the trace's other path switches are tests/chain_path_scenes.py's.

Materials differ between all triangles of a scene (colour, emission and smoothness from the index), so that a wrong
winner changes the pixel.  They stay ordinary here (smoothness and colours in [0, 1]); material edges live in
tests/material_scenes.py."""
from __future__ import annotations

import math

import numpy as np

import raytracingc_amd as rt
from raytracingc_amd._abi import TRIANGLE_DT, RtcCamera, Vec3

U = 2.0 ** -24
# rtc_prep_primary: sane needs ed = 4 * 9.006 u |AB|_1 |AC|_1 < 2.5e-4, so the switch is at this |AB|_1 |AC|_1
SANE_PRODUCT = 2.5e-4 / (4.0 * 9.006 * U)
# ball_of: a cluster is cullable only while edRatio = 8 u E^2 rhoMax / EPSILON < 0.5 (rhoMax = 4, EPSILON = 0.001)
ED_RATIO_EDGE = math.sqrt(0.5 * 0.001 / (8.0 * U * 4.0))
EPSILON = 0.001
CLUSTER = 8


# ---- building blocks ---------------------------------------------------------------------------------------------
def _v(p):
    return np.asarray(p, np.float64)


def tri(a, b, c, normal=None, toward=(0.0, 0.0, 0.0)):
    """One triangle as a tuple (A, B, C, N); without `normal` the unit geometric normal on the side of `toward`."""
    a, b, c = _v(a), _v(b), _v(c)
    if normal is None:
        n = np.cross(b - a, c - a)
        ln = np.linalg.norm(n)
        n = n / ln if ln > 0 and np.isfinite(ln) else np.array([0.0, 0.0, -1.0])
        if np.dot(n, _v(toward) - (a + b + c) / 3.0) < 0:
            n = -n
        normal = n
    return a, b, c, _v(normal)


def quad(p, e1, e2, **kw):
    """Two triangles over the parallelogram p, p + e1, p + e1 + e2, p + e2."""
    p, e1, e2 = _v(p), _v(e1), _v(e2)
    return [tri(p, p + e1, p + e1 + e2, **kw), tri(p, p + e1 + e2, p + e2, **kw)]


def box(centre, size):
    """12 triangles, normals outwards."""
    c, h = _v(centre), 0.5 * size
    out = []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            n = np.zeros(3)
            n[axis] = sgn
            a1, a2 = np.zeros(3), np.zeros(3)
            a1[(axis + 1) % 3], a2[(axis + 2) % 3] = 2 * h, 2 * h
            p = c + n * h - 0.5 * a1 - 0.5 * a2
            out += quad(p, a1, a2, normal=n)
    return out


def floor(y=2.0, x0=-6.0, x1=6.0, z0=0.25, z1=9.0):
    return quad((x0, y, z0), (x1 - x0, 0, 0), (0, 0, z1 - z0), normal=(0.0, -1.0, 0.0))


def material(i):
    """(colour, emission, smoothness) of triangle i: distinct for i < 1001."""
    return ((0.25 + 0.07 * (i % 11), 0.9 - 0.06 * (i % 13), 0.3 + 0.1 * (i % 7)), 0.5 * (i % 3), 0.25 * (i % 4))


def build(rows, offset=(0.0, 0.0, 0.0)) -> np.ndarray:
    """Triangle[] of (A, B, C, N) rows, vertices shifted by `offset` in double and rounded to float32."""
    t = np.zeros(len(rows), TRIANGLE_DT)
    off = _v(offset)
    with np.errstate(all="ignore"):
        for i, (a, b, c, n) in enumerate(rows):
            for key, p in (("posA", a + off), ("posB", b + off), ("posC", c + off), ("normal", n)):
                t[i][key] = tuple(np.asarray(p, np.float64).astype(np.float32))
            col, em, sm = material(i)
            t[i]["mat"]["color"] = col
            t[i]["mat"]["emissionStrength"] = em
            t[i]["mat"]["smoothness"] = sm
    return t


def camera(origin=(0.0, 0.0, 0.0), looking_at=(0.0, 0.0, 1.0), fov=1.0) -> RtcCamera:
    return rt.camera_basis(tuple(origin), tuple(looking_at), fov)


def camera_with(cam: RtcCamera, fov=None, ex_scale=None) -> RtcCamera:
    """A copy of `cam` with another fov, or with ex scaled (a caller-supplied basis that is not unit)."""
    c = RtcCamera()
    c.origin, c.ex, c.ey, c.ez, c.fov = cam.origin, cam.ex, cam.ey, cam.ez, cam.fov
    if fov is not None:
        c.fov = fov
    if ex_scale is not None:
        c.ex = Vec3(cam.ex.x * ex_scale, cam.ex.y * ex_scale, cam.ex.z * ex_scale)
    return c


def cluster_order(tris) -> np.ndarray:
    """rtc_scene.hip split_clusters restated: the triangle indices in cluster order (cluster k = entries 8k..8k+7): recursive
    stable sorts of the centroids A + (AB + AC) / 3 (AB, AC float32 differences) along their longest extent, NaN last."""
    f = lambda k: np.stack([tris[k][c] for c in "xyz"], 1)  # noqa: E731
    with np.errstate(all="ignore"):
        A, B, C = f("posA"), f("posB"), f("posC")
        cen = A.astype(np.float64) + ((B - A).astype(np.float64) + (C - A).astype(np.float64)) / 3.0

    def split(idx):
        n = len(idx)
        if n <= CLUSTER:
            return idx
        c = cen[idx]
        with np.errstate(all="ignore"):
            ext = [np.max(c[~np.isnan(c[:, a]), a], initial=-1e300) - np.min(c[~np.isnan(c[:, a]), a], initial=1e300)
                   for a in range(3)]
        axis = 0
        for a in (1, 2):
            if ext[a] > ext[axis]:
                axis = a
        key = np.where(np.isnan(c[:, axis]), 1e300, c[:, axis])
        idx = [idx[k] for k in np.argsort(key, kind="stable")]
        leaves = (n + CLUSTER - 1) // CLUSTER
        mid = (leaves + 1) // 2 * CLUSTER
        return split(idx[:mid]) + split(idx[mid:])

    return np.array(split(list(range(len(tris)))), np.int64)


# ---- the base mesh: a box on a floor in front of a wall, seen from the origin along +z (16 triangles) ----------------
def base_mesh():
    return (box((0.0, 0.9, 4.0), 1.6) + floor(1.75)
            + quad((-5.0, -3.5, 8.0), (10.0, 0, 0), (0, 6.0, 0), normal=(0.0, 0.0, -1.0)))


SCENES: dict = {}


def _add(name, rows, cam, note, offset=(0.0, 0.0, 0.0)):
    assert name not in SCENES
    SCENES[name] = (build(rows, offset), cam, note)


# ---- coplanar_ties ---------------------------------------------------------------------------------------------------
# Each scene: a pair of overlapping coplanar triangles with different materials, P0 at index 0 and P1 at index 9; six
# small fillers far left and two far right make x the split axis and put P1 (centroid left of P0's, except in
# ties_rotated) into cluster 0 and P0 into cluster 1: the cluster walk meets the higher index first.  A diffuse floor below sends bounce rays at them.
def _ties(p0, p1):
    left = [tri((-5.6 + 0.3 * k, -2.0 + 0.5 * k, 5.0), (-5.4 + 0.3 * k, -2.0 + 0.5 * k, 5.0), (-5.5 + 0.3 * k, -1.7 + 0.5 * k, 5.0))
            for k in range(6)]
    right = [tri((5.2, -1.0 + k, 5.0), (5.6, -1.0 + k, 5.0), (5.4, -0.6 + k, 5.0)) for k in range(2)]
    fl = floor(1.75, -4.0, 4.0, 0.25, 4.0)  # (its two centroids: x = 4/3 and x = -4/3; glossy: 0.5 and 0.75)
    #       0     1-6    7       8          9   10      11
    rows = [p0] + left + [fl[1]] + right[:1] + [p1, fl[0]] + right[1:]
    return rows


# ties_axis: AB = (8, 0, 0) and AC = (., 4, 0) in z = 4, so det = -32 dir.z and dot(AC, q) = 32 (pos - A).z are exact
# scalings by a power of two for both triangles, from any origin: equal dst bit for bit wherever both are hit
_add("ties_axis", _ties(tri((-3.5, -2.75, 4.0), (4.5, -2.75, 4.0), (1.0, 1.25, 4.0)),
                        tri((-4.0, -2.5, 4.0), (4.0, -2.5, 4.0), (0.0, 1.5, 4.0))),
     camera(), "coplanar_ties: two triangles in z = 4, different vertices; filter active")
# the plane z = 4 + y / 2: the same edges along x, AC = (., 4, 2)
_add("ties_tilted", _ties(tri((-3.5, -2.5, 2.75), (4.5, -2.5, 2.75), (1.5, 1.5, 4.75)),
                          tri((-4.0, -2.5, 2.75), (4.0, -2.5, 2.75), (0.0, 1.5, 4.75))),
     camera(), "coplanar_ties: two triangles in a tilted plane; filter active")
_TA, _TB, _TC = (-4.0, -2.5, 4.0), (4.0, -2.5, 4.0), (0.0, 1.5, 4.0)
_add("ties_rotated", _ties(tri(_TA, _TB, _TC), tri(_TB, _TC, _TA)),
     camera(), "coplanar_ties: one triangle twice, vertices rotated A,B,C -> B,C,A; filter active")


# ---- slivers -----------------------------------------------------------------------------------------------------
# Needles along the frame's middle row (dy = 0: y = 0 exactly for every ray of it) and middle column, whose |det| =
# 2 area * |dir.z| crosses EPSILON across the frame, and two big triangles seen edge-on: their planes pass through the
# middle row's (column's) rays at z = 4 with a slope chosen so that |det| = 0.0015 |dir.z| there.
def _needle_x(x0, x1, z, w):  # along x, centred on y = 0, width w
    return tri((x0, -0.5 * w, z), (x1, -0.5 * w, z), (0.5 * (x0 + x1), 0.5 * w, z))


def _needle_y(y0, y1, z, w, x=0.0):
    return tri((x - 0.5 * w, y0, z), (x - 0.5 * w, y1, z), (x + 0.5 * w, 0.5 * (y0 + y1), z))


def slivers_mesh():
    s = 0.0015 / 36.0  # the edge-on triangles' 2 * area is 36
    return [
        _needle_x(-1.0, 1.0, 1.5, 2e-3),       # aspect 1e3: 2 area 4e-3, visible where it is
        _needle_x(-4.0, 4.0, 2.5, 1.9e-4),     # aspect 4e4: 2 area 1.52e-3, |det| crosses EPSILON at |dx| ~ 1.1
        _needle_x(-5.0, 5.0, 3.0, 1.0e-4),     # aspect 1e5: 2 area 1.0e-3: |det| at EPSILON in the middle, below elsewhere
        _needle_x(-20.0, 20.0, 12.0, 4.0e-5),  # aspect 1e6: 2 area 1.6e-3
        _needle_y(-0.9, 0.9, 1.25, 1.8e-3),    # aspect 1e3, the middle column
        _needle_y(-3.0, 3.0, 3.5, 3.0e-4),     # aspect 2e4: 2 area 1.8e-3, crosses EPSILON at |dy| ~ 0.75
        # edge-on, the middle row: the plane y = s (z - 4), geometric normal (dir.y = 0 there: dot(dir, N) = -s dir.z)
        tri((-9.0, -s, 3.0), (9.0, -s, 3.0), (0.0, s, 5.0)),
        # edge-on, the middle column: the plane x = s (z - 4.5)
        tri((-s, -9.0, 3.5), (-s, 9.0, 3.5), (s, 0.0, 5.5)),
    ] + base_mesh()


_add("slivers", slivers_mesh(), camera(), "slivers: aspect 1e3 to 1e6 and edge-on triangles; filter active; oversized edges")


# ---- near_eps ------------------------------------------------------------------------------------------------------
# Five unit-sized triangles at z = 0.0005 .. 0.002 in front of the camera, each covering the frame right of dx = its edge:
# dst = z / dir.z lies on both sides of EPSILON over the frame
def near_eps_mesh():
    rows = []
    for z, dx in ((0.0005, 0.9), (0.0008, 0.3), (0.001, -0.3), (0.0012, -0.9), (0.002, -1.5)):
        rows.append(tri((dx * z, -1.0, z), (dx * z, 1.0, z), (dx * z + 1.0, 0.0, z), normal=(0.0, 0.0, -1.0)))
    return rows + base_mesh()


_add("near_eps", near_eps_mesh(), camera(), "near_eps: dst on both sides of EPSILON; filter active")


# ---- origin_in_plane ---------------------------------------------------------------------------------------------------
# dAC0 == 0 (the `never` path): the origin in a triangle's plane, on a vertex of another, on an edge of a third
_O = (0.5, -0.25, 0.125)
def origin_in_plane_mesh():
    o = _v(_O)
    return [
        tri(o + (-1.0, 0.0, 2.0), o + (1.0, 0.0, 2.0), o + (0.0, 0.0, 5.0), normal=(0.0, -1.0, 0.0)),  # plane y = o.y
        tri(o, o + (1.0, 0.5, 3.0), o + (-1.0, 0.5, 3.0), normal=(0.0, -1.0, 0.0)),                   # A = origin
        tri(o + (-0.5, -0.5, -1.0), o + (0.5, 0.5, 1.0), o + (2.0, -1.0, 2.0)),                       # origin = (A + B) / 2
        tri(o + (-2.0, -1.0, 0.0), o + (-2.0, 1.0, 0.0), o + (-2.0, 0.0, 3.0), normal=(1.0, 0.0, 0.0)),  # not in plane
    ] + [(a + o, b + o, c + o, n) for a, b, c, n in base_mesh()]


_add("origin_in_plane", origin_in_plane_mesh(), camera(_O, _v(_O) + (0.0, 0.0, 1.0)),
     "origin_in_plane: dAC0 == 0 for three triangles; filter active")


# ---- far_offset --------------------------------------------------------------------------------------------------------
for _name, _off in (("far_offset_1e3", (1024.0, -768.0, 1536.0)), ("far_offset_1e5", (98304.0, -65536.0, 131072.0))):
    _add(_name, slivers_mesh(), camera(_off, _v(_off) + (0.0, 0.0, 1.0)),
         "far_offset: the slivers and the base mesh translated with the camera; filter active; oversized edges", offset=_off)


# ---- mixed_scale -------------------------------------------------------------------------------------------------------
def _right(p, l1, l2, **kw):  # legs along x and y at p, facing -z
    p = _v(p)
    return tri(p, p + (l1, 0.0, 0.0), p + (0.0, l2, 0.0), normal=(0.0, 0.0, -1.0), **kw)


def mixed_scale_mesh():
    lo, hi = math.sqrt(SANE_PRODUCT * 0.98), math.sqrt(SANE_PRODUCT * 1.02)  # legs: |AB|_1 |AC|_1 = leg^2
    rows = [
        _right((-11.5, -6.0, 30.0), lo, lo),   # 0: sane
        _right((0.5, -6.0, 30.0), hi, hi),     # 1: not sane
        _right((-0.3, -0.3, 2.0), 1e-3, 1e-3), _right((0.2, -0.4, 2.0), 1e-3, 1e-3), _right((0.1, 0.3, 2.0), 1e-3, 1e-3),
        _right((-9.0, -7.5, 32.0), ED_RATIO_EDGE * 0.99, 6.0),   # 5: longest edge just below the edRatio switch
        _right((-9.0, -15.0, 32.0), ED_RATIO_EDGE * 1.01, 6.0),   # 6: just above
    ]
    rows += quad((-5e3, 1.75, -5e3), (1e4, 0, 0), (0, 0, 1e4), normal=(0.0, -1.0, 0.0))  # 7, 8: the 1e4 floor
    rows += [
        tri((0.0, 0.0, 50.0), (1e19, 0.0, 50.0), (0.0, -1e19, 50.0), normal=(0.0, 0.0, -1.0)),   # 9
        tri((0.0, 0.0, 60.0), (-1e30, 0.0, 60.0), (0.0, -1e30, 60.0), normal=(0.0, 0.0, -1.0)),  # 10
    ]
    return rows + box((0.0, 0.9, 4.0), 1.6)


OVERSIZED = {"mixed_scale": (9, 10)}  # the 1e19 and 1e30 triangles
_add("mixed_scale", mixed_scale_mesh(), camera(),
     "mixed_scale: 1e-3 to 1e30; sane straddle (0 below, 1 above); oversized")


# ---- bad_normals -------------------------------------------------------------------------------------------------------
def bad_normals_mesh():
    g = np.array([0.0, 0.0, -1.0])
    t = math.radians(89.9)
    normals = [
        (0.0, 0.0, 0.0), (math.nan, math.nan, math.nan), (0.0, 0.0, -math.inf), (0.0, 0.0, math.inf),
        tuple(1e-3 * g), tuple(1e3 * g), tuple(-g), (-math.sin(t), 0.0, -math.cos(t)),
        (0.0, math.nan, -1.0), (math.inf, 0.0, -1.0), tuple(g), tuple(g),
    ]
    rows = []
    for k, n in enumerate(normals):  # a 4 x 3 grid of unit-sized triangles in z = 3.5
        x, y = -2.4 + 1.2 * (k % 4), -1.6 + 1.1 * (k // 4)
        rows.append(tri((x, y, 3.5), (x + 1.1, y, 3.5), (x + 0.5, y + 1.0, 3.5), normal=n))
    return rows + base_mesh()


NAN_NORMALS = {"bad_normals": (1, 8)}
_add("bad_normals", bad_normals_mesh(), camera(),
     "bad_normals: zero, NaN, inf, non-unit, opposite and 89.9 degrees off; misaligned; filter active")


# ---- nonfinite ---------------------------------------------------------------------------------------------------------
def nonfinite_mesh():
    b = base_mesh()
    odd = [
        tri((-1.0, -1.0, 3.0), (math.nan, -1.0, 3.0), (-0.5, 0.0, 3.0), normal=(0.0, 0.0, -1.0)),   # a NaN vertex
        tri((1.0, -1.0, 3.0), (2.0, math.inf, 3.0), (1.5, 0.0, 3.0), normal=(0.0, 0.0, -1.0)),      # a +inf vertex
        tri((0.3, -0.2, 3.0), (0.3, -0.2, 3.0), (0.3, -0.2, 3.0), normal=(0.0, 0.0, -1.0)),         # A = B = C
        tri((-0.4, -0.6, 3.0), (-0.4, -0.6, 3.0), (0.4, -0.9, 3.0), normal=(0.0, 0.0, -1.0)),       # A = B
    ]
    # between the ordinary triangles, in index order and in space
    return b[:3] + odd[:1] + b[3:7] + odd[1:2] + b[7:10] + odd[2:3] + b[10:13] + odd[3:] + b[13:]


DEGENERATE = {"nonfinite": (3, 8, 12, 16)}
_add("nonfinite", nonfinite_mesh(), camera(), "nonfinite: NaN and inf vertices, zero-area triangles; degenerate")


# ---- counts ------------------------------------------------------------------------------------------------------------
def grid_mesh(nx=6, ny=6):
    """2 nx ny triangles: a bumpy sheet in front of the camera (heights from fixed arithmetic)."""
    h = lambda i, j: 4.0 + 0.125 * ((i * 7 + j * 3) % 5)  # noqa: E731
    rows = []
    for j in range(ny):
        for i in range(nx):
            p = lambda a, b: (-2.4 + 0.8 * a, -2.0 + 0.7 * b, h(a, b))  # noqa: E731
            rows.append(tri(p(i, j), p(i + 1, j), p(i + 1, j + 1)))
            rows.append(tri(p(i, j), p(i + 1, j + 1), p(i, j + 1)))
    return rows


COUNTS = (1, 7, 8, 9, 63, 64, 65)
for _n in COUNTS:
    _add(f"counts_{_n}", grid_mesh()[:_n], camera(), f"counts: the grid mesh cut to {_n} triangles; filter active")


# ---- chunks ------------------------------------------------------------------------------------------------------------
def chunks_mesh():
    """The slivers mesh (24 triangles) on a 4 x 3 grid: 288 triangles, 36 clusters, 2 chunks."""
    rows = []
    for j in range(3):
        for i in range(4):
            off = _v((-7.5 + 5.0 * i, -4.0 + 4.0 * j, 2.0 + 1.5 * ((i + 2 * j) % 3)))
            rows += [(a + off, b + off, c + off, n) for a, b, c, n in slivers_mesh()]
    return rows


_add("chunks", chunks_mesh(), camera((0.0, 0.0, -6.0), (0.0, 0.0, 1.0)),
     "chunks: 288 triangles, more than 32 clusters; filter active; oversized edges")


# ---- cameras ---------------------------------------------------------------------------------------------------------
def _far_basis():
    return camera((3.0, -2.5, -1.0), (-0.7, 1.1, 4.3), 0.8)


for _base in ("slivers", "mixed_scale"):
    _t, _c, _note = SCENES[_base]
    _act = "; filter active" if "filter active" in _note else ""
    _extra = "".join(f"; {k}" for k in ("sane straddle (0 below, 1 above)", "oversized") if k in _note)
    for _tag, _cam, _what in (
            ("fov_0.02", camera_with(_c, fov=0.02), "fov 0.02"),
            ("fov_3", camera_with(_c, fov=3.0), "fov 3.0"),
            # (its rays fan out in the plane z = 4 through the box and the floor)
            ("fov_1e-7", camera((-6.0, 0.5, 4.0), (-6.0, 0.5, 5.0), 1e-7), "fov 1e-7 (K.vmin > 1e-6 false: no tile is prefiltered)"),
            ("ex_x2", camera_with(_c, ex_scale=2.0), "ex scaled by 2 (unitBasis false: no tile is prefiltered)"),
            ("far_basis", _far_basis(), "a basis far from the axes")):
        # (a sane-straddle claim holds for the scene's own camera; the camera variants do not repeat it)
        SCENES[f"{_base}_{_tag}"] = (_t, _cam, f"cameras: {_base} with {_what}"
                                     + (_act if _tag in ("fov_3", "far_basis") else "")
                                     + ("; oversized" if "oversized" in _extra else ""))

for _k in OVERSIZED.copy():
    for _name in list(SCENES):
        if _name.startswith(_k + "_"):
            OVERSIZED[_name] = OVERSIZED[_k]
