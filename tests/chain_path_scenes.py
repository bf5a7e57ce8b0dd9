"""Geometry on both sides of rtc_render_chain's path switches ("the trace's path switches"), as plain data like
tests/adversarial_scenes.py: SCENES maps a name to (Triangle[] as TRIANGLE_DT, RtcCamera, note), FRAMES a frame name to
(scene, width, height, spp, maxBounce).  Fixed arithmetic, no random draws; the materials differ between all triangles of a
scene, so a wrong winner changes the pixel.  Every note names the path its scene is for; tests/test_chain_path_scenes.py
shows each claim with the CPU oracle alone, tests/test_gpu_chain_paths.py renders the frames on every route.

The switches (rtc_chain.h chain_trace_pairs, rtc_render.hip size_chain_lds / run_chain), nCl = clusters = ceil(T / 8):
  table   first bounce of a single-chunk scene (nCl <= 32) with the cluster cull on: the clusters with a record reachable
          from the primary hit point p0 (nLive of them) are tabulated once per window;
  fused   table and 64 nLive <= 1024 (kChainPairs): the cull and the pair list in one pass.  nLive >= 17 takes the
          separate cull and pair build, whose list overflows (a window of 64 live lanes keeping every live cluster enters
          64 nLive > 1024 pairs) and is flushed through the pair passes in the middle of the build;
  dense   later bounces of a single-chunk scene with at most 16 (kDenseCullMax) live lanes: up to 16 x 32 culls taken 64
          at a time; more live lanes take the per-lane loop, which the HITS kernel replaces by fusedG while
          64 nCl <= 1024 -- so HITS scenes of nCl >= 17 run the per-lane loop with its own overflow flush;
  MULTI   nCl >= 33: chunk by chunk, records from global memory;
  chainPrimF  the primary filter records are staged in LDS while the block's LDS stays within its share of the CU's.

chainPrimF, derived.  size_chain_lds stages them when  kChainStaticLds + recLds + pfLds <= kCuLds / wgsPerCu  with
  kChainStaticLds = sizeof(PowTablesLds) + 4 sizeof(ChainWaveLds) + 64 + 32 sizeof(DevCluster)
                  = (16 x 2 x 8 + 32 x 8) + 4 x (32 x 2 x 16 + 64 x 8 + 1024 x 2 + 64 x 16) + 64 + 32 x 32
                  = 512 + 4 x 4608 + 64 + 1024 = 20,032 bytes,
  recLds = soa_slots(8 nCl) sizeof(DevTri) = 512 nCl,   pfLds = triPadded sizeof(DevPrimF) = 64 x 8 nCl = 512 nCl
(triPadded = 8 ceil(T / 8) = 8 nCl), kCuLds = 163,840: staged exactly when 20,032 + 1,024 nCl <= 163,840 / wgsPerCu.
  4 workgroups per CU (hit-heavy scenes' whole frames): 40,960 -> nCl <= 20.  The smallest unstaged single-chunk scene has
    21 clusters, T = 161 (box_primf_4); its neighbour below is T = 160 (box_primf_4_below, 20 clusters).
  3 workgroups per CU (every other launch): 54,613 -> nCl <= 33, and a single-chunk scene has at most 32: no single-chunk
    scene runs unstaged at 3 workgroups per CU.  (A scene of 33 clusters is MULTI, which never stages.)  So "box_primf_3"
    does not exist; what can be pinned at 3 is that the largest single-chunk scene (layers_32, 52,800 bytes) and
    box_primf_4 itself -- as a small row share, which runs RTC_CHAIN_WGS_SHARE = 3 -- are staged.
A hit-heavy scene therefore runs the HITS kernel (no GENERAL code) with nCl > 16 only for 17 <= nCl <= 20: box_diffuse_T
has T = 144, 18 clusters."""
from __future__ import annotations

import math

import numpy as np

from adversarial_scenes import ED_RATIO_EDGE, build, camera, quad

CLUSTER, CHUNK_CLUSTERS, CHAIN_PAIRS, DENSE_CULL_MAX = 8, 32, 1024, 16
WGS_HIT_SHARE = 0.15  # kWgsHitShare: above it a scene's whole frames run 4 workgroups per CU and the HITS kernel
# size_chain_lds, restated (the derivation above)
CHAIN_STATIC_LDS = (16 * 2 * 8 + 32 * 8) + 4 * (32 * 2 * 16 + 64 * 8 + 1024 * 2 + 64 * 16) + 64 + 32 * 32
CU_LDS = 160 * 1024


def clusters_of(tri_count):
    return (tri_count + CLUSTER - 1) // CLUSTER


def prim_f_staged(tri_count, wgs_per_cu):
    """size_chain_lds' P.chainPrimF for a scene of tri_count triangles."""
    n = clusters_of(tri_count)
    return n <= CHUNK_CLUSTERS and CHAIN_STATIC_LDS + 512 * n + 64 * CLUSTER * n <= CU_LDS // wgs_per_cu


def first_unstaged(wgs_per_cu):
    """The smallest single-chunk triangle count that runs with the primary filter records in global memory; None: none."""
    for t in range(1, CHUNK_CLUSTERS * CLUSTER + 1):
        if not prim_f_staged(t, wgs_per_cu):
            return t
    return None


SCENES: dict = {}
FRAMES: dict = {}


def _add(name, tris, cam, note):
    assert name not in SCENES
    tris.setflags(write=False)
    SCENES[name] = (tris, cam, note)


# ---- layers_N --------------------------------------------------------------------------------------------------------
# A floor patch at y = 1 (+y is down: the camera at the origin looks along +z and sees it below the horizon) under N
# horizontal layers at y_k = -(1 + k / 2), k = 0 .. N - 1, stored normal (0, 1, 0): they are hit from below.  A layer is a
# star of 8 needles through (0, y_k, 4): 18 long (every needle has an edge > ED_RATIO_EDGE = 16.2, so ball_of gives its
# cluster the never-cull escape), 0.25 wide at the thick end, turned by pi / 8 from needle to needle and by a
# layer-dependent phase, each shifted sideways by up to 0.1.  Layer 0 has six needles; with the floor's two triangles it
# makes a cluster of 8.  8 N triangles, N clusters.
# Grouping (rtc_build_clusters: stable median splits of the centroids along their longest extent): a needle's centroid
# is within 0.3 of its layer's axis point and the floor's two are 1.33 apart, the layers 0.5 apart in y and the floor 2
# below layer 0, so every split is along y and cuts between layers: cluster c is layer N - 1 - c, the last one layer 0 and
# the floor.  For N = 33 that last cluster is the second chunk.  (tests/test_chain_path_scenes.py checks the grouping the
# library builds, not this paragraph.)
# From a floor point p0 every needle's winding is reachable (dot(AC, (p0 - A) x AB) > 0: AB x AC points down at the
# floor), so all N clusters are live in table mode; with the never-cull escape every live lane keeps all of them.
LAYER_CENTRE_Z, LAYER_HALF_LENGTH, LAYER_WIDTH, LAYER_STEP = 4.0, 9.0, 0.25, 0.5


def _needle(k, j):
    th = (j + (k * 5 % 8) / 8.0) * math.pi / 8.0
    u, v = np.array([math.cos(th), 0.0, math.sin(th)]), np.array([-math.sin(th), 0.0, math.cos(th)])
    c = np.array([0.0, -(1.0 + LAYER_STEP * k), LAYER_CENTRE_Z]) + v * (0.05 * ((j * 3 + k) % 5 - 2))
    a, b = c - LAYER_HALF_LENGTH * u, c + LAYER_HALF_LENGTH * u
    tip = c + (0.3 * ((j + k) % 3 - 1)) * u + LAYER_WIDTH * v
    # (A, tip, B): AB x AC = (.. u + 0.25 v) x 18 u = 4.5 (v x u) = (0, 4.5, 0), down at the floor
    return a, tip, b, np.array([0.0, 1.0, 0.0])


def layers_mesh(n):
    rows = []
    for k in range(n - 1, -1, -1):
        rows += [_needle(k, j) for j in range(8 if k else 6)]
    return rows + quad((-2.0, 1.0, 2.0), (4.0, 0, 0), (0, 0, 4.0), normal=(0.0, -1.0, 0.0))


def layers_tris(n):
    """The floor's two triangles (the last two) get a colour with a component 1: p = max(rayColor) = 1 at the primary hit is
    never below the roulette draw, so every sample of a floor pixel goes on to a first bounce -- a full window has 64 live
    lanes there, 64 nLive pairs.  (60 live lanes x 17 clusters would still fit the list.)"""
    t = build(layers_mesh(n))
    for i, col in ((len(t) - 2, (1.0, 0.625, 0.375)), (len(t) - 1, (1.0, 0.5, 0.75))):
        t[i]["mat"]["color"] = col
    return t


LAYERS = (16, 17, 32, 33)
_LAYER_NOTES = {
    16: "the last fused table build: nLive = 16, 64 x 16 = 1024 pairs fill the list exactly",
    17: "the separate cull and pair build: nLive = 17, the 1024-entry list overflows once per full window",
    32: "the separate build at the single-chunk maximum: nLive = 32, one flush per 16 clusters; 52,800 bytes of LDS, "
        "staged at 3 workgroups per CU",
    33: "MULTI: two chunks, the last of one cluster (layer 0 and the floor)",
}
for _n in LAYERS:
    _add(f"layers_{_n}", layers_tris(_n), camera(),
         f"layers: {_n} clusters, every one oversized (never culled) and reachable from every floor point; "
         f"{_LAYER_NOTES[_n]}; not hit-heavy")
    FRAMES[f"layers_{_n}"] = (f"layers_{_n}", 48, 40, 64, 4)


# ---- boxes -------------------------------------------------------------------------------------------------------------
# A closed box about the origin, half extents (2, 1.5, 2.5), seen from inside: every face a grid of (nu, nv) quads, two
# triangles each, the stored normals and the windings (AB x AC) pointing inwards.  Every bounce ray hits again: hit-heavy.
BOX_HALF = (2.0, 1.5, 2.5)


def box_mesh(grids, grow=0.0):
    """The faces -x, +x, -y, +y, -z, +z with grids[f] = (nu, nv) quads; half extents BOX_HALF + grow."""
    h, rows = np.array(BOX_HALF) + grow, []
    for f, (nu, nv) in enumerate(grids):
        axis, sgn = f // 2, (-1.0, 1.0)[f % 2]
        b, c = (axis + 1) % 3, (axis + 2) % 3
        inward = np.zeros(3)
        inward[axis] = -sgn

        def p(i, j):
            q = np.zeros(3)
            q[axis], q[b], q[c] = sgn * h[axis], (2.0 * i / nu - 1.0) * h[b], (2.0 * j / nv - 1.0) * h[c]
            return q

        for j in range(nv):
            for i in range(nu):
                for t in ((p(i, j), p(i + 1, j), p(i + 1, j + 1)), (p(i, j), p(i + 1, j + 1), p(i, j + 1))):
                    if np.dot(np.cross(t[1] - t[0], t[2] - t[0]), inward) < 0:
                        t = (t[0], t[2], t[1])
                    rows.append((t[0], t[1], t[2], inward))
    return rows


def split_last(rows):
    """One more triangle: the last one cut from A to the midpoint of BC (both halves keep its winding)."""
    a, b, c, n = rows[-1]
    m = 0.5 * (b + c)
    return rows[:-1] + [(a, b, m, n), (a, m, c, n)]


BOX_CAMERA = ((0.3, -0.2, -0.5), (1.0, 0.4, 2.0), 1.0)
# 6 x (4 x 3) quads = 144 triangles, 18 clusters
_add("box_diffuse_T", build(box_mesh([(4, 3)] * 6)), camera(*BOX_CAMERA),
     "box_diffuse_T: T = 144, 18 clusters, single chunk, hit-heavy and staged at 4 workgroups per CU: the HITS kernel "
     "without fusedG (64 x 18 > 1024); colours below 1, so the roulette ends paths after 1..maxBounce hits and a "
     "window's later bounces pass from more than 16 live lanes (per-lane loop) to 16 or fewer (dense cull, nCl > 16)")
# 2 x (4 x 4) + 4 x (4 x 3) quads = 160 triangles, 20 clusters; one triangle cut in two: 161, 21 clusters
_GRIDS_160 = [(4, 4), (4, 4), (4, 3), (4, 3), (4, 3), (4, 3)]
_add("box_primf_4_below", build(box_mesh(_GRIDS_160)), camera(*BOX_CAMERA),
     "box_primf_4_below: T = 160, 20 clusters: the largest hit-heavy scene whose primary filter records are staged at 4 "
     "workgroups per CU (40,512 <= 40,960 bytes)")
_add("box_primf_4", build(split_last(box_mesh(_GRIDS_160))), camera(*BOX_CAMERA),
     "box_primf_4: T = 161, 21 clusters: the smallest single-chunk scene that runs !chainPrimF (41,536 > 40,960 bytes at "
     "4 workgroups per CU): a GENERAL kernel even pipelined; staged again as a small row share (3 per CU)")


def _shiny(smoothness):
    """Two 12-triangle boxes, one 0.5 outside the other, with colour (1, 1, 1): p = max(rayColor) = 1 is never below the
    roulette draw (< 1), and the division by p leaves rayColor (1, 1, 1): every sample makes exactly maxBounce hits.
    Emissions differ by triangle.  (One shell alone leaks: a hit within EPSILON of an edge has its next hit, on the
    adjacent face, closer than EPSILON, which rayTriangle rejects -- the oracle shows samples of 17 hits at maxBounce 63.
    Such a ray now hits the outer shell, is reflected and re-enters through the inner one, whose stored normals face
    inwards: rayTriangle is one-sided in the stored normal.)"""
    t = build(box_mesh([(1, 1)] * 6) + box_mesh([(1, 1)] * 6, grow=0.5))
    for c in "xyz":
        t["mat"]["color"][c] = 1.0
    t["mat"]["emissionStrength"] = (0.01 * (1 + np.arange(len(t)))).astype(np.float32)
    t["mat"]["smoothness"] = smoothness
    return t


_add("box_mirror", _shiny(1.0), camera(*BOX_CAMERA),
     "box_mirror: two shells of 12 triangles, smoothness 1, colour 1: h == maxBounce for every sample; with maxBounce >= 64 every lane "
     "has lane + iter >= nAct in the late iterations (computed draws, rng_jump_by(7 iter)) and hq > 64 leaves the window: "
     "one sample per window")
_add("box_gloss", _shiny(0.75), camera(*BOX_CAMERA),
     "box_gloss: box_mirror with smoothness 0.75: h == maxBounce all the same, and every bounce direction depends on its "
     "draws, so a wrong computed draw or a wrong lane in the walk changes the pixel (the mirror's samples are all equal)")
MIRROR_BOUNCES = (63, 64, 65, 100)

FRAMES["box_diffuse_T"] = ("box_diffuse_T", 24, 20, 64, 10)
FRAMES["box_primf_4_below"] = ("box_primf_4_below", 24, 20, 16, 6)
FRAMES["box_primf_4"] = ("box_primf_4", 24, 20, 16, 6)
for _mb in MIRROR_BOUNCES:
    FRAMES[f"box_mirror_mb{_mb}"] = ("box_mirror", 16, 8, 5, _mb)
    FRAMES[f"box_gloss_mb{_mb}"] = ("box_gloss", 16, 8, 5, _mb)
# mixed h, about ten windows per pixel, nAct < 64 in the last ones (est = need * jn / k with few samples left)
FRAMES["box_diffuse_deep"] = ("box_diffuse_T", 16, 8, 130, 40)

# two passes split inside a window (tests/test_gpu_chain_paths.py): scene, width, height, maxBounce; 37 + 27 samples
PASS_SPLIT = (37, 27)
PASS_FRAMES = {"layers_17": ("layers_17", 48, 40, 4), "box_diffuse_T": ("box_diffuse_T", 24, 20, 10),
               "box_mirror_mb65": ("box_mirror", 16, 8, 65), "box_gloss_mb65": ("box_gloss", 16, 8, 65)}

assert ED_RATIO_EDGE < 2 * LAYER_HALF_LENGTH
