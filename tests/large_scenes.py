"""Scenes of 16,385 to 393,217 triangles, as plain data: the size classes at which the loops and allocations that
scale with the triangle count first take another turn, each the smallest count that crosses its boundary.

  name      T        words  clusters  chunks
  w257      16,385     257     2,049      65   past one stride of the tile cull's workgroup (256 words) and one ballot word
                                               of chunks (64)
  cap       393,216  6,144    49,152   1,536   the tile cull's cap (rtc_plan.h kMaxCullMaskWords): its largest LDS request
  past_cap  393,217  6,145    49,153   1,537   the first scene that renders without the tile cull and rtc_render_chain

field(T) is a height field of two triangles per cell, twice as wide as deep, seen from above, and one more triangle, the
awning.  Nothing is drawn at random and nothing is read from a file.  Triangle i < T - 1 lies in cell perm(i // 2), perm
being the multiplication by a fixed unit modulo the cell count: neighbours on the screen come from all over the index
range, so every tile's candidates spread over low and high mask words and the cluster build has to regroup them.  The
materials differ between all triangles of a scene (the colour components run through three pairwise coprime moduli);
smoothness and emission stay ordinary.

The relief (world: +y is down in the image, the camera's up is -y): square pits of two by two cells between walls that rise
WALL cell sides over one cell.  A flat field returns almost no bounce ray; from these pits the diffuse bounce of a hit lands
on geometry again about as often as it leaves (tests/test_large_scenes.py holds the counts).  A cell's side is
0.09 * sqrt(2) at every size: rayTriangle's `det < EPSILON` rejects much smaller cells for every ray.

The awning is triangle T - 1: level, LIFT above the floor of the pits, over the field's last corner and reaching far
beyond it, with a stored normal that lies level and points back over the field (rayTriangle is one-sided in the stored
normal only: the awning is seen from above and hit from below by whatever leaves the pits outwards).  Its centroid is the
last one along x and along z and nowhere near the ends of y, so the cluster build's median splits leave it in the last
cluster.  At 16,385 and 393,217 triangles it is the one triangle of the last mask word and of the last cluster and chunk:
there the two boundaries of the class are this triangle, which a good part of the frame sees and bounces onto.

FRAME is a class's render launch, QUERY the launch whose primary rays and recorded bounce rays are its query rays; the
camera stands over the middle of the field, high enough for the launch's aspect, and MARGIN is chosen so that the corner
pixels of the 33 x 17 launch still land on the field's first and last cells (chunk 0 is a patch of some ten by fifteen
cells in a field of 628 by 314)."""
from __future__ import annotations

import functools
import math

import numpy as np

import oracle.binding as orc
import raytracingc_amd as rt
import trace_rays_reference as tr
from primary_rays import launch_rays
from raytracingc_amd._abi import TRIANGLE_DT

CLASSES = {"w257": 16385, "cap": 393216, "past_cap": 393217}
CLUSTER, CHUNK = 8, 32  # triangles per cluster, clusters per chunk
# (width, height, spp, maxBounce) of a class's frames, and (width, height) of the launch behind its query rays
FRAME = {"w257": (48, 40, 3, 4), "cap": (33, 17, 2, 4), "past_cap": (33, 17, 2, 4)}
QUERY = {"w257": (64, 40), "cap": (33, 17), "past_cap": (33, 17)}
SIDE = 0.09  # the field's area is SIDE^2 * T: a cell's side stays 0.09 * sqrt(2) at every size
PIT_CELLS = 4  # the relief's period in cells, along x and along z
WALL = 2.5  # a wall's height in cell sides: it rises over one cell, at atan(WALL) = 68 degrees
LIFT = 0.8  # the awning's height above the pits' floors
MARGIN = 1.005  # the camera's height over what shows the whole field
TILT = 0.02  # the camera stands this much of its height before the point it looks down at (its basis needs a horizon)
RHO_SCALE = 3.0  # replay directions times this have |dir|_1 beyond kClusterRhoMax = 4 (tests/trace_rays_reference.py)


def counts(T):
    """(padded triangles, mask words, clusters, chunks) of T triangles."""
    padded = (T + CLUSTER - 1) // CLUSTER * CLUSTER
    clusters = padded // CLUSTER
    return padded, (padded + 63) // 64, clusters, (clusters + CHUNK - 1) // CHUNK


def _unit(n):
    """The fixed unit modulo n: the first number from round(0.618 n) upwards that is coprime to n."""
    u = max(int(round(0.6180339887 * n)), 1)
    while math.gcd(u, n) != 1:
        u += 1
    return u


def grid(T):
    """(cells, columns, rows, cell side) of field(T), twice as wide as deep; the last row may be partial."""
    cells = T // 2  # (the last triangle is the awning)
    nx = int(math.ceil(math.sqrt(2.0 * cells)))
    return cells, nx, (cells + nx - 1) // nx, SIDE * math.sqrt(2.0)


def height(ix, iz):
    """The relief at grid vertex (ix, iz) in cell sides, upwards: pits of PIT_CELLS - 2 cells between walls."""
    return np.where((ix % PIT_CELLS == 0) | (iz % PIT_CELLS == 0), WALL, 0.0)


@functools.lru_cache(maxsize=None)
def field(T):
    """Triangle[T] as TRIANGLE_DT, read-only."""
    cells, nx, nz, c = grid(T)
    i = np.arange(T, dtype=np.int64)
    cell = (i // 2) * _unit(cells) % cells
    cx, cz = cell % nx, cell // nx
    second = (i % 2).astype(bool)

    def vertex(dx, dz):
        ix, iz = cx + dx, cz + dz
        return np.stack([(ix - 0.5 * nx) * c, -c * height(ix, iz), (iz - 0.5 * nz) * c], 1)

    p00, p10, p11, p01 = vertex(0, 0), vertex(1, 0), vertex(1, 1), vertex(0, 1)
    A = p00
    B = np.where(second[:, None], p11, p10)
    C = np.where(second[:, None], p01, p11)
    xe, ze = 0.5 * nx * c, 0.5 * nz * c
    A[-1], B[-1], C[-1] = (xe - 5.0, -LIFT, ze + 1.0), (xe + 1.0, -LIFT, ze - 5.0), (xe + 8.5, -LIFT, ze + 8.5)
    n = np.cross(B - A, C - A)
    n /= np.linalg.norm(n, axis=1)[:, None]
    n[n[:, 1] > 0] *= -1.0  # the stored normal points up (-y): every ray arrives from above a height field
    n[-1] = (-math.sqrt(0.5), 0.0, -math.sqrt(0.5))
    t = np.zeros(T, TRIANGLE_DT)
    for key, v in (("posA", A), ("posB", B), ("posC", C), ("normal", n)):
        for k, a in enumerate("xyz"):
            t[key][a] = v[:, k].astype(np.float32)
    # distinct below 61 * 67 * 71 * 7 = 2,031,239 triangles
    t["mat"]["color"]["x"] = (0.30 + 0.65 * (i % 61) / 60.0).astype(np.float32)
    t["mat"]["color"]["y"] = (0.95 - 0.65 * (i % 67) / 66.0).astype(np.float32)
    t["mat"]["color"]["z"] = (0.30 + 0.65 * (i % 71) / 70.0).astype(np.float32)
    t["mat"]["emissionStrength"] = (0.5 * (i % 7 % 3)).astype(np.float32)
    t["mat"]["smoothness"] = (0.25 * (i % 7 % 4)).astype(np.float32)
    t.setflags(write=False)
    return t


def camera_args(T, width, height_, shift=(0.0, 0.0, 0.0)):
    """camera_basis' arguments: above the field, looking down on all of it, for a launch of width x height_ pixels; `shift`
    moves the camera, not what it looks at."""
    _, nx, nz, c = grid(T)
    aspect = (width // 2) / (height_ // 2)
    h = MARGIN * max(0.5 * nx * c / aspect, 0.5 * nz * c)
    return (0.0 + shift[0], -h + shift[1], -TILT * h + shift[2]), (0.0, 0.0, 0.0), 1.0


@functools.lru_cache(maxsize=None)
def camera(T, width, height_):
    return rt.camera_basis(*camera_args(T, width, height_))


# ---- a class's data, each computed once and read-only ----------------------------------------------------------------------
def tris(name):
    return field(CLASSES[name])


def frame_camera(name):
    return camera(CLASSES[name], *FRAME[name][:2])


def query_camera(name):
    return camera(CLASSES[name], *QUERY[name])


def frame_config(name, **route):
    W, H, spp, mb = FRAME[name]
    return rt.RenderConfig(W, H, spp, mb, True, **route)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def records(name):
    """rt.scene_records_host of the class's triangles."""
    rec = rt.scene_records_host(tris(name))
    _frozen(*rec.values())
    return rec


@functools.lru_cache(maxsize=None)
def cluster_slot(name):
    """int64 [T]: where the cluster order (the clTris records) keeps reference triangle i."""
    ref = records(name)["clTris"][:, 12].view(np.int32)
    slot = np.full(CLASSES[name], -1, np.int64)
    slot[ref[ref >= 0]] = np.flatnonzero(ref >= 0)
    assert (slot >= 0).all()
    return _frozen(slot)[0]


@functools.lru_cache(maxsize=None)
def frame_oracle(name, row_start=0, row_stride=1, row_band=0):
    """The oracle's (u8, floats, segments) of the class's frame, or of a row share of it."""
    d = frame_config(name, row_start=row_start, row_stride=row_stride, row_band=row_band).desc()
    col, acc, seg = orc.render(tris(name), None, rt.default_scene(), frame_camera(name), d, threads=16)
    _frozen(col, acc)
    return col, acc, seg


@functools.lru_cache(maxsize=None)
def launch_primary(name, which):
    """RAY_DT [W * H]: the primary rays of the class's frame ("frame") or of its query launch ("query")."""
    W, H = FRAME[name][:2] if which == "frame" else QUERY[name]
    return _frozen(launch_rays(camera(CLASSES[name], W, H), rt.RenderConfig(W, H, 0, 0, True)))[0]


@functools.lru_cache(maxsize=None)
def replay_calls(name):
    """The oracle's records (oracle.binding.CALL_DT) of every calculateRayCollision call after a pixel's first, rendering
    the class's query launch with seeds x + y * width and maxBounce 10: tests/trace_rays_reference.replay_calls'
    construction."""
    rays = launch_primary(name, "query")
    n = len(rays)
    with np.errstate(all="ignore"):
        _, _, calls, ncalls = orc.calc_path(tris(name), None, rt.default_scene(), 1, rays, np.arange(n, dtype=np.uint32),
                                            np.full(n, 10, np.int32))
    k = np.arange(calls.shape[1])[None, :]
    return _frozen(calls[(k >= 1) & (k < ncalls[:, None])].copy())[0]


@functools.lru_cache(maxsize=None)
def query_rays(name):
    """RAY_DT [n]: the query launch's primary rays, its replay rays and the replay rays with dir times 3 (beyond the
    cluster bound), under a fixed permutation."""
    calls = replay_calls(name)
    rays = np.concatenate([launch_primary(name, "query"), tr.rays_of(calls), tr.rays_of(calls, RHO_SCALE)])
    return _frozen(rays[np.random.default_rng(20240611).permutation(len(rays))])[0]


@functools.lru_cache(maxsize=None)
def expected(name, which):
    """tr.expected of launch_primary(name, "frame" / "query") or query_rays(name) ("rays")."""
    rays = query_rays(name) if which == "rays" else launch_primary(name, which)
    return tr.expected(tris(name), None, 1, rays)
