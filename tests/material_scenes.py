"""Materials outside the range every other scene keeps to (smoothness in [0, 1], colours in [0, 1], emission <= 10), as
plain data like tests/chain_path_scenes.py: SCENES maps a name to (Triangle[] as TRIANGLE_DT, RtcCamera, note),
SPHERE_SCENES a name to (Triangle[], Sphere[], RtcCamera, note), FRAMES a frame name to (scene, width, height, spp,
maxBounce).  Fixed arithmetic, no random draws.  The reference clamps none of these values (objloader.c gives
smoothness = sqrt(0.001 Ns) for any Ns, triangles.txt takes any decimal), so calcColor's arithmetic on them is part of
what the kernels must reproduce bit for bit.  tests/test_material_scenes.py shows every claim of a note with the CPU oracle
alone, tests/test_gpu_materials.py renders the frames on every route; tests/golden/kat_calc_materials.npz pins the oracle to
the reference's own calcColor on the finite scenes (through its text format) and kat_ref_materials.npz on every scene, the
non-finite ones and the sphere scenes included (as raw records; tests/reference_calc.py).

What the values reach (rtc_chain.h chain_trace_pairs, rtc_lane.h, rtc_sky.h):
  smoothness  ray.dir = lerp(diffuseDir, specularDir, smoothness) is not unit and extrapolates outside [0, 1]; reflect keeps
              the length, so |dir| grows by about |s| per bounce.  The cluster cull, the first bounce's table mode and the
              chunk cull are proved for |dir|_1 <= kClusterRhoMax = 4 only and are gated on it (rhoOk; the table by a ballot
              over the wave's live lanes).  dst is the ray parameter and shrinks as 1 / |dir|: from |dir| ~ size / EPSILON
              on every hit has dst < EPSILON, the ray leaves a closed box and the environment sees a huge direction.
  colour      p = max(rayColor) decides the roulette (p < draw ends the path) and divides rayColor: p = +0 and -0, p > 1
              (never ends a path), p < 0, NaN components (fmax drops them), p = NaN and p = inf (inf * 0 = NaN).
  emission    3e38 makes a sample inf, the accumulator inf and, across samples, inf - inf = NaN: the deferred slots, the
              in-kernel sums, the passes' accumulator reload and the u8 conversion all see them.

The sky: the ladder's frames are rendered with sunFocus 0 (SKY below says why), every other frame under the default Scene.

Windings equal the stored normals (AB x AC along the normal) in every scene, as the reference's parseAndPlaceTriangle
recomputes them: the scenes go through its text format unchanged (tests/golden/make_golden.py asserts it)."""
from __future__ import annotations

import math

import numpy as np

from adversarial_scenes import base_mesh, build, camera
from chain_path_scenes import BOX_CAMERA, box_mesh, layers_mesh
from sphere_scenes import OPEN5_ROWS, spheres

SCENES: dict = {}
SPHERE_SCENES: dict = {}
FRAMES: dict = {}
ORDINARY: dict = {}  # scene -> the same geometry with adversarial_scenes.material(i) on every triangle


def recomputed_normals(tris):
    """raytracing.c:24, normalized(cross(minus(B, A), minus(C, A))), in float32 as the reference forms it (moremath.c:7-17: the
    sum of squares in float, sqrt and 1 / length in double, each rounded to float).  The scenes store these bits -- not the
    exact axis a mesh was built with, from which they may differ in the last place -- so that the reference's text format
    gives back the same Triangle[]."""
    f = np.float32
    g = lambda k: np.stack([tris[k][c] for c in "xyz"], 1).astype(f)  # noqa: E731
    u, v = (g("posB") - g("posA")).astype(f), (g("posC") - g("posA")).astype(f)
    c = np.stack([((u[:, 1] * v[:, 2]).astype(f) - (u[:, 2] * v[:, 1]).astype(f)).astype(f),
                  ((u[:, 2] * v[:, 0]).astype(f) - (u[:, 0] * v[:, 2]).astype(f)).astype(f),
                  ((u[:, 0] * v[:, 1]).astype(f) - (u[:, 1] * v[:, 0]).astype(f)).astype(f)], 1)
    sq = (c * c).astype(f)
    length = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(f) + sq[:, 2]).astype(f).astype(np.float64)).astype(f)
    n = (c * (1.0 / length.astype(np.float64)).astype(f)[:, None]).astype(f)
    out = tris.copy()
    for k, a in enumerate("xyz"):
        out["normal"][a] = n[:, k]
    return out


def _add(name, tris, cam, note, ordinary):
    assert name not in SCENES
    tris, ordinary = recomputed_normals(tris), recomputed_normals(ordinary)
    tris.setflags(write=False)
    ordinary.setflags(write=False)
    SCENES[name] = (tris, cam, note)
    ORDINARY[name] = ordinary


# ---- the smoothness ladder --------------------------------------------------------------------------------------------
# Three closed geometries seen from inside (chain_path_scenes.box_mesh and its camera), every triangle with the ladder's
# smoothness and a colour whose x is 1: p = max(rayColor) = 1 is never below the draw and the division by p leaves
# rayColor.x = 1, so the roulette never ends a path and every sample goes on until maxBounce or until it leaves the box.
#   shell  two shells of 12 triangles (chain_path_scenes._shiny's): 3 clusters, hit-heavy: the HITS kernel's fusedG
#   boxT   box_diffuse_T's 6 x (4 x 3) quads: 144 triangles, 18 clusters: the HITS kernel's per-lane loop and the dense cull
#   fine   6 x (5 x 5) quads: 300 triangles, 38 clusters, two chunks: MULTI and its chunk cull
LADDER = {"m1": -1.0, "2": 2.0, "2p5": 2.5, "8": 8.0, "1e6": 1e6, "3e38": 3e38}
_LADDER_NOTES = {
    "m1": "extrapolation on the diffuse side: rho mostly below 4 at the first bounce, growing later",
    "2": "first-bounce waves with a few lanes beyond rho = 4: the table mode is dropped for the whole wave because of them",
    "2p5": "mixed waves at the first bounce, later bounces from 4 up to size / EPSILON: every cull runs with rhoOk on both sides",
    "8": "almost every lane beyond 4 from the first bounce on",
    "1e6": "every second-bounce hit has dst < EPSILON: the ray leaves the closed box and the environment sees |dir| ~ 1e6",
    "3e38": "inf and NaN directions",
}
GEOMETRIES = {
    "shell": (lambda: box_mesh([(1, 1)] * 6) + box_mesh([(1, 1)] * 6, grow=0.5), "shell: 24 triangles, 3 clusters, fusedG"),
    "boxT": (lambda: box_mesh([(4, 3)] * 6), "boxT: 144 triangles, 18 clusters, the per-lane loop then the dense cull"),
    "fine": (lambda: box_mesh([(5, 5)] * 6), "fine: 300 triangles, 38 clusters, MULTI"),
}


def ladder_tris(rows, smoothness):
    t = build(rows)
    t["mat"]["color"]["x"] = 1.0
    t["mat"]["smoothness"] = smoothness
    # (material(i)'s other values repeat after 273 triangles)
    t["mat"]["emissionStrength"] += (0.125 * (np.arange(len(t)) // 273)).astype(np.float32)
    return t


for _g, (_mesh, _gnote) in GEOMETRIES.items():
    for _tag, _s in LADDER.items():
        _add(f"{_g}_s{_tag}", ladder_tris(_mesh(), _s), camera(*BOX_CAMERA),
             f"{_gnote}; smoothness {_s:g}: {_LADDER_NOTES[_tag]}; hit-heavy", build(_mesh()))

# layers_17 (chain_path_scenes: 17 oversized clusters over a floor, the separate cull and pair build with a list flush, not
# hit-heavy) with smoothness 2.5 on the floor's two triangles, whose colours keep their component 1
_l17 = build(layers_mesh(17))
for _i, _col in ((len(_l17) - 2, (1.0, 0.625, 0.375)), (len(_l17) - 1, (1.0, 0.5, 0.75))):
    _l17[_i]["mat"]["color"] = _col
_l17o = _l17.copy()
_l17["mat"]["smoothness"][-2:] = 2.5
_add("layers17_s2p5", _l17, camera(), "layers17: layers_17 with smoothness 2.5 on the floor: first-bounce windows of 17 live "
     "clusters with lanes on both sides of rho = 4; not hit-heavy", _l17o)


# ---- colour and emission edges ------------------------------------------------------------------------------------------
# (colour, emission or None: material(i)'s, smoothness or None) on every fourth triangle, in turn; the other triangles keep
# adversarial_scenes.material(i), so a wrong winner still changes the pixel
_N, _I = math.nan, math.inf
EDGES = {
    "zero": [((0.0, 0.0, 0.0), None, None), ((-0.0, -0.0, -0.0), None, None), ((-0.0, 0.0, -0.0), None, None),
             ((0.0, -0.0, 0.0), None, None)],
    "bright": [((4.0, 0.5, 2.0), None, None), ((1.5, 1.5, 1.5), None, None), ((1.0, 1e-30, 1e30), None, None)],
    "negative": [((-0.5, -0.25, -2.0), 1.0, None), ((-1.0, 0.5, 0.25), -1.0, None), ((-0.5, -0.25, -2.0), -1.0, None),
                 ((-1.0, 0.5, 0.25), 1.0, None)],
    "blinding": [((2.0, 1.0, 0.5), 3e38, None), ((-1.0, 0.5, 0.25), 3e38, None)],
    "nonfinite": [((_N, 0.5, 0.75), None, None), ((0.5, _I, 0.25), None, None), ((_N, _N, _N), None, None),
                  ((_I, _I, _I), None, None), ((0.5, 0.75, 1.0), _N, None), ((0.5, 0.75, 1.0), _I, None),
                  ((1.0, 0.5, 0.75), -_I, None), ((0.75, 1.0, 0.5), None, _N), ((1.0, 0.75, 0.5), None, _I),
                  ((_N, -0.5, -0.25), None, None), ((0.25, 0.5, -_I), None, None), ((-0.5, _N, -0.25), 1.0, None)],
}
EVERY = 4


def edge_tris(rows, kind, every=EVERY, first=0):
    t = build(rows)
    return put_edges(t, kind, every, first)


def put_edges(t, kind, every, first):
    for k, i in enumerate(range(first, len(t), every)):
        col, em, sm = EDGES[kind][k % len(EDGES[kind])]
        t[i]["mat"]["color"] = col
        if em is not None:
            t[i]["mat"]["emissionStrength"] = em
        if sm is not None:
            t[i]["mat"]["smoothness"] = sm
    return t


def open_mesh():
    """adversarial_scenes.base_mesh (a box on a floor in front of a wall, seen from the origin: sky above and beside the
    wall) and two smaller boxes beside it: 40 triangles, 5 clusters, open -- bounce rays miss as often as they hit."""
    from adversarial_scenes import box
    rows = base_mesh() + box((-2.2, 1.15, 3.2), 1.1) + box((2.1, 1.3, 2.9), 0.8)
    # (adversarial_scenes winds freely -- rayTriangle is two-sided in the winding --; here AB x AC follows the normal)
    return [(a, b, c, n) if np.dot(np.cross(b - a, c - a), n) > 0 else (a, c, b, n) for a, b, c, n in rows]


def _edges(rows, kind, nonfinite_every):
    """nonfinite is thinned out to each of its materials once (they turn almost every path that meets them into NaN, and
    NaN positions are left out of the comparisons); bright and negative materials on triangles 2, 6, 10, .. beside them
    keep the finite pixels apart from the ordinary materials' frame."""
    if kind != "nonfinite":
        return edge_tris(rows, kind)
    t = put_edges(put_edges(build(rows), "bright", 8, 2), "negative", 8, 6)
    return put_edges(t, "nonfinite", nonfinite_every, 0)


NONFINITE_EVERY = {"cbox": 12, "copen": 3}  # 144 and 40 triangles: 12 and 14 places for the 12 materials
for _kind in EDGES:
    _where = "once each, bright and negative ones between them" if _kind == "nonfinite" else "on every fourth triangle"
    _add(f"cbox_{_kind}", _edges(box_mesh([(4, 3)] * 6), _kind, NONFINITE_EVERY["cbox"]), camera(*BOX_CAMERA),
         f"cbox: box_diffuse_T's geometry with the {_kind} materials {_where}; hit-heavy", build(box_mesh([(4, 3)] * 6)))
    _add(f"copen_{_kind}", _edges(open_mesh(), _kind, NONFINITE_EVERY["copen"]), camera(),
         f"copen: an open scene over a floor with the {_kind} materials {_where}: bounce rays miss more often than they "
         f"hit, yet hit-heavy by the upload's measure (share 0.30)",
         build(open_mesh()))


# ---- spheres ----------------------------------------------------------------------------------------------------------------
# sphere_scenes.open5's layout beside the ultracomplex model, one sphere per kind: the mirror ball bright with smoothness
# 2.5, the glossy one negative (emission -1) with smoothness 8, the lamp blinding (emission 3e38), the one behind the
# camera a zero (-0, +0, -0); the huge ground sphere, which most pixels see, is bright grey (p = 1.5: the roulette
# never ends a path there).  In spheres_nonfinite the glossy sphere is nonfinite instead (a NaN and an inf colour component,
# emission inf).  So inf and NaN reach the sphere material loads at the primary hit and later, the split launch's sums and the
# passes' reload.
MATERIAL5_ROWS = [
    (OPEN5_ROWS[0][0], OPEN5_ROWS[0][1], (4.0, 0.5, 2.0), 0.0, 2.5),
    (OPEN5_ROWS[1][0], OPEN5_ROWS[1][1], (-1.0, 0.5, 0.25), -1.0, 8.0),
    (OPEN5_ROWS[2][0], OPEN5_ROWS[2][1], (2.0, 1.0, 0.5), 3e38, 0.0),
    (OPEN5_ROWS[3][0], OPEN5_ROWS[3][1], (1.5, 1.5, 1.5), 0.0, 0.0),
    (OPEN5_ROWS[4][0], OPEN5_ROWS[4][1], (-0.0, 0.0, -0.0), 0.0, 0.0),
]
# from the model's other side, nearer than the default camera: the mirror ball and the lamp are seen directly
SPHERE_CAMERA = ((3.5, -2.0, -3.0), (0.3, -1.2, 1.2), 1.2)
NONFINITE_SPHERE = (OPEN5_ROWS[1][0], OPEN5_ROWS[1][1], (_N, 0.5, _I), _I, 8.0)


def sphere_scene(name):
    """(triangles, spheres, camera, note) of SPHERE_SCENES, built on first use (the triangles are a golden scene's)."""
    if name not in SPHERE_SCENES:
        import raytracingc_amd as rt
        from conftest import load_tris

        tris = load_tris("ultracomplex")[0]
        s = spheres(MATERIAL5_ROWS)
        if name == "spheres_open":
            note = "spheres_open: the open five-sphere layout: the split launch"
        elif name == "spheres_nonfinite":
            s = spheres(MATERIAL5_ROWS[:1] + [NONFINITE_SPHERE] + MATERIAL5_ROWS[2:])
            note = "spheres_nonfinite: spheres_open with a nonfinite glossy sphere: the split launch"
        elif name == "spheres_closed":
            # (a closing sphere alone leaves the upload's bounce-hit share below the split's gate: rays from its inside
            # count as leaving; a box of triangles seen from inside does not)
            tris = np.concatenate([tris, build(box_mesh([(1, 1)] * 6, grow=90.0), offset=(0.0, 30.0, 0.0))])
            note = "spheres_closed: spheres_open inside a closed box of 12 triangles: one lane per pixel"
        else:
            raise KeyError(name)
        tris.setflags(write=False)
        s.setflags(write=False)
        SPHERE_SCENES[name] = (tris, s, rt.camera_basis(*SPHERE_CAMERA), note)
    return SPHERE_SCENES[name]


SPHERE_NAMES = ("spheres_open", "spheres_closed", "spheres_nonfinite")
SPHERE_FRAME = (48, 40, 32, 10)  # width, height, spp, maxBounce

# ---- frames ---------------------------------------------------------------------------------------------------------------
# computed draws past the window (maxBounce 65: every window commits one sample) with long directions
FRAMES["shell_s2p5_mb65"] = ("shell_s2p5", 16, 8, 5, 65)
FRAMES["layers17_s2p5"] = ("layers17_s2p5", 48, 40, 64, 4)
# smoothness 1e6: that EVERY sample's environment sees |dir|_1 > 1e5 cannot hold over many samples -- the diffuse direction
# falls within 0.1 of the specular one in about 0.35 % of them, and dir = 1e6 (specular - diffuse) + diffuse -- so these
# frames are small (768 samples, the smallest |dir|_1 is 1.116e5) and hold for the pixels, seeds and camera they have: a
# change of any of them may need another shape.  Each of their paths is a primary hit and an environment evaluation;
# boxT_s1e6_full below, held to no such claim, carries the load (30,720 samples).
# The three geometries share their planes, so at 8, 1e6 and 3e38 -- where rays soon hit nothing more -- their frames differ
# in the primary hit's material and in the kernel that renders them, not in the paths.
# 3e38: 16 samples keep the NaN pixels (one NaN sample is enough) below half the frame
_LADDER_SHAPES = {"1e6": (24, 16, 2), "3e38": (24, 20, 16)}
for _g in GEOMETRIES:
    for _tag in LADDER:
        FRAMES[f"{_g}_s{_tag}"] = (f"{_g}_s{_tag}", *_LADDER_SHAPES.get(_tag, (24, 20, 64)), 6 if _g == "fine" else 10)
for _kind in EDGES:
    FRAMES[f"cbox_{_kind}"] = (f"cbox_{_kind}", 24, 20, 64, 10)
    FRAMES[f"copen_{_kind}"] = (f"copen_{_kind}", 48, 40, 16, 6)

# The sky.  A direction of |dir| > 56 gives powf(dot(dir, sun), 22) = inf, and below the horizon (dir.y >= 0, sunMask 0)
# inf * 0 = NaN: under the reference's sun nearly every pixel of a ladder frame is NaN from smoothness 2 on, and with the
# sun at the zenith (dot(dir, sun) = -dir.y, positive only above the horizon) nearly every pixel is +inf -- frames that
# no wrong winner could change.  So the ladder is rendered with sunFocus 0: powf(x, 0) = 1 for every x, the sun term is
# sunIntensity above the horizon, and the frames stay finite and differ pixel by pixel.  Two frames keep focus 22 under
# the zenith sun for the overflowing powf itself: all but saturated with +inf, never NaN.
SKY = {f: dict(focus=0.0) for f in FRAMES if f.startswith(("shell_", "boxT_", "fine_"))}
FRAMES["boxT_s1e6_full"] = ("boxT_s1e6", 24, 20, 64, 10)
FRAMES["boxT_s8_sun"] = ("boxT_s8", 24, 20, 16, 10)
SKY.update(boxT_s1e6_full=dict(sun=(0.0, -1.0, 0.0)), boxT_s8_sun=dict(sun=(0.0, -1.0, 0.0)))
# 3e38: "inf and then NaN" is the sun term's (with focus 0 the frames have neither); the sun tilted by 1 : 50 from the
# zenith leaves the NaN to a sliver of directions, and 16 samples keep the NaN pixels below half the frame
SKY.update({f: dict(sun=(0.0, -50.0, 1.0)) for f in FRAMES if f.endswith("_s3e38")})


def sky(frame):
    """The Scene a frame is rendered under: the reference's default with SKY's changes."""
    import raytracingc_amd as rt

    return rt.default_scene(**SKY.get(frame, {}))


FRAMES["cbox_nonfinite"] = ("cbox_nonfinite", 24, 20, 4, 6)  # (few samples and bounces: in the closed box most paths go NaN)
NAN_FRAMES = tuple(f for f in FRAMES if f.endswith(("_blinding", "_nonfinite", "_s3e38")))  # an accumulator may hold NaN

# two passes split inside a window: scene, width, height, maxBounce; 37 + 27 samples (chain_path_scenes.PASS_SPLIT)
PASS_FRAMES = {"boxT_s2p5": ("boxT_s2p5", 24, 20, 10), "cbox_blinding": ("cbox_blinding", 24, 20, 10)}
