"""The checker that ties the launch planner's model to the device, and the matrix of launches it is run on.

The planner (raytracingc_amd/csrc/rtc_plan.h) declares what every kernel of a launch touches: footprint rows of (op, res,
access, id, lo, hi).  tests/test_plan*.py prove on a model of HIP streams that kernels which may run together touch
disjoint declared memory; this module checks the other half -- that what a launch CHANGES in the scene's memory lies
where its own plan declares a write.  Plain numpy, no GPU: tests/test_footprints.py proves the checker on synthetic
snapshots and the matrix's intent on the planner's CPU hooks, tests/test_gpu_footprints.py runs the matrix on the device
(DeviceScene.last_plan: the plan the executor ran; DeviceScene.spans: every allocation of the scene).

    allowed_ranges(plan_rows, spans, pool_taken)   the write, atomic and keyed-write rows as byte ranges per span
    violations(before, after, allowed)             the changed bytes outside them

A snapshot is a list of uint8 arrays, one per span (empty where nothing is allocated).  A diff sees a byte only when its
value changes: a byte rewritten with its old value, and every read, is invisible to it."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np

import raytracingc_amd as rt
import test_plan

READ, WRITE, ATOMIC, KEYED_WRITE = 0, 1, 2, 3
WRITES = (WRITE, ATOMIC, KEYED_WRITE)
TRAILER = np.uint64(2 ** 64 - 1)
# rtc_plan.h Res: the resources a scene owns (rtc_scene_spans lists them), and the caller's
RES_SCRATCH, RES_PRIM, RES_GEOSET, RES_SAMPLES, RES_SEGSLOTS, RES_SCENE_GEN = 0, 1, 2, 3, 4, 9
RES_DRAW_TABLE, RES_ITEM_DRAW, RES_MEMBERSHIP, RES_DRAW_POOL = 12, 13, 18, 21
SCENE_RES = {RES_SCRATCH: "scratch", RES_PRIM: "prim", RES_GEOSET: "geoset", RES_SAMPLES: "samples",
             RES_SEGSLOTS: "segslots", RES_SCENE_GEN: "scene_gen", RES_DRAW_TABLE: "draw_table",
             RES_ITEM_DRAW: "item_draw", RES_MEMBERSHIP: "membership", RES_DRAW_POOL: "draw_pool"}
DRAW_CTR_PART, DRAW_BLOCK_BYTES = 1, 1024  # rtc_layout.h DrawCtr kDcTaken is word 0 of part 1; kDrawBlockBytes
# rtc_plan.h Kernel and Res by name: tests/test_plan.py's tables, with the kernels and resources behind them (as
# tests/test_plan_render_pixels.py extends them)
KNAMES = test_plan.KNAMES[:14] + ["regroup_centroids", "regroup_level", "regroup_index", "render_pixels"]
RES_NAMES = test_plan.RES_NAMES[:18] + ["membership", "regroup_scratch", "pixel_list"]
REGIONS = ["mask", "pixMask", "weight", "order", "geoList", "superMask", "pixItem", "geoColor"]  # rtc_plan.h Buf
# A kernel's scratch write rows come in kTouches' order, and a launch that binds a later one of them binds the earlier
# ones (pixItem: merge, which implies the lists), so the k-th scratch write row of a kernel names its region
# (tests/test_footprints.py holds this against rtc_plan_sim_regions for every case of the matrix)
SCRATCH_WRITES = {"super_cull": ["superMask"], "tile_cull": ["mask", "pixMask", "weight", "geoList", "pixItem"],
                  "chain": ["geoColor"], "order": ["order"]}
SLOTS, GEO_RING, SPAN_COUNT = 8, 16, 60


# ---- the checker --------------------------------------------------------------------------------------------------------
def split_plan(ops, rows):
    """(ops, footprint rows, trailer) of a plan as DeviceScene.last_plan or a planner hook hands it back."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 6)
    assert len(rows) and rows[-1][0] == TRAILER, "the plan's last row is its ~0 record"
    return np.asarray(ops).reshape(-1, 4), rows[:-1], rows[-1]


def allowed_ranges(plan_rows, spans, pool_taken=None):
    """{span index: [(lo, hi), ...]} -- where the plan's write, atomic and keyed-write rows allow a byte of the scene's
    memory to change.  A scratch row is its [lo, hi) inside the scratch span; a unit row [0, 1) is the whole of every span
    of its (res, id); rows of the caller's resources name no span.  The draw cache's pool is in no row: a launch whose
    plan writes the draw table (its tile cull takes blocks) may write the blocks from `pool_taken` on, the number taken
    before it, and no launch the blocks below."""
    spans = np.asarray(spans, np.uint64).reshape(-1, 5)
    allowed = {}
    takes_blocks = False
    for row in np.asarray(plan_rows, np.uint64).reshape(-1, 6):
        _, res, access, ident, lo, hi = (int(v) for v in row)
        if access not in WRITES:
            continue
        takes_blocks |= res == RES_DRAW_TABLE
        for i, (sres, sid, _, _, sbytes) in enumerate(spans):
            if int(sres) != res or res not in SCENE_RES:
                continue
            if res == RES_SCRATCH:
                assert lo <= hi <= int(sbytes), f"a scratch row [{lo}, {hi}) outside the scratch's {int(sbytes)} bytes"
                allowed.setdefault(i, []).append((lo, hi))
            elif int(sid) == ident:
                assert (lo, hi) == (0, 1), "a row outside the scratch is one unit"
                allowed.setdefault(i, []).append((0, int(sbytes)))
    if takes_blocks and pool_taken is not None:
        for i, (sres, _, _, _, sbytes) in enumerate(spans):
            if int(sres) == RES_DRAW_POOL:
                allowed.setdefault(i, []).append((min(int(pool_taken) * DRAW_BLOCK_BYTES, int(sbytes)), int(sbytes)))
    return allowed


def changed(before, after):
    """Per span, the offsets of the bytes that differ."""
    assert len(before) == len(after)
    out = []
    for b, a in zip(before, after):
        assert b.shape == a.shape, "a span changed its size between the snapshots"
        out.append(np.flatnonzero(b != a))
    return out


def violations(before, after, allowed, diff=None):
    """[(span index, byte offset), ...]: every changed byte outside the allowed ranges (diff: changed(before, after) where
    the caller has it already)."""
    bad = []
    for i, off in enumerate(changed(before, after) if diff is None else diff):
        ok = np.zeros(len(off), bool)
        for lo, hi in allowed.get(i, []):
            ok |= (off >= lo) & (off < hi)
        bad += [(i, int(o)) for o in off[~ok]]
    return bad


def scratch_write_rows(ops, plan_rows):
    """[(region name, lo, hi)] of the plan's scratch write rows, named by SCRATCH_WRITES."""
    out, seen = [], {}
    for row in plan_rows:
        i, res, access, _, lo, hi = (int(v) for v in row)
        if res != RES_SCRATCH or access not in WRITES:
            continue
        kernel = KNAMES[int(ops[i][3])]
        k = seen.get(i, 0)
        seen[i] = k + 1
        out.append((SCRATCH_WRITES[kernel][k], lo, hi))
    return out


def written_names(ops, plan_rows, spans, before, after, diff=None):
    """The names of what shows a changed byte inside a declared write: scratch regions by name, the resources outside the
    slot by SCENE_RES's names (the non-vacuity half of the GPU test)."""
    spans = np.asarray(spans, np.uint64).reshape(-1, 5)
    diff = changed(before, after) if diff is None else diff
    names = set()
    scratch = [i for i, s in enumerate(spans) if int(s[0]) == RES_SCRATCH]
    for name, lo, hi in scratch_write_rows(ops, plan_rows):
        if any(((diff[i] >= lo) & (diff[i] < hi)).any() for i in scratch):
            names.add(name)
    for i, s in enumerate(spans):
        if int(s[0]) != RES_SCRATCH and len(diff[i]):
            names.add(SCENE_RES[int(s[0])])
    return names


def pool_taken(spans, snapshot, reset):
    """The draw cache's blocks taken when `snapshot` was made (the first counter word), 0 when the launch clears the cache
    first (`reset`: the plan's trailer says the launch regrew or cleared something) or nothing is allocated yet."""
    for i, s in enumerate(np.asarray(spans, np.uint64).reshape(-1, 5)):
        if int(s[0]) == RES_DRAW_TABLE and int(s[2]) == DRAW_CTR_PART and len(snapshot[i]) >= 4 and not reset:
            return int(snapshot[i][:4].view(np.uint32)[0])
    return 0


# ---- the matrix ---------------------------------------------------------------------------------------------------------
CUBE_CAMERAS = (((-4.0, -3.08, 0.0), (0.0, -1.58, 0.0), 3.5), ((-3.7, -3.0, 0.4), (0.0, -1.58, 0.0), 3.5),
                ((-4.2, -2.9, -0.3), (0.0, -1.58, 0.0), 3.5))
LAYER_CAMERAS = (((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 1.0), ((0.1, 0.0, 0.05), (0.0, 0.0, 1.0), 1.0),
                 ((-0.1, 0.0, -0.05), (0.0, 0.0, 1.0), 1.0))


LARGE_SCENE_SIZES = {"w257": (48, 40), "cap": (33, 17), "past_cap": (33, 17)}  # the frames of tests/large_scenes.py


def _default_cameras():
    o = rt.DEFAULT_ORIGIN
    return tuple((tuple(np.add(o, d)), rt.DEFAULT_LOOKING_AT, rt.DEFAULT_FOV)
                 for d in ((0, 0, 0), (0.3, 0.1, 0.2), (-0.2, -0.1, 0.3)))


@functools.lru_cache(maxsize=None)
def geometry(scene):
    """(triangles, spheres or None, three cameras as camera_basis arguments: the case's, and the two dirtying launches')."""
    from chain_path_scenes import SCENES as PATH_SCENES
    from conftest import load_tris, scene_spheres
    from sphere_scenes import open5

    if scene == "layers_33":
        return PATH_SCENES[scene][0], None, LAYER_CAMERAS
    if scene in LARGE_SCENE_SIZES:  # (tests/large_scenes.py: the case's camera sees the whole field, the others stand aside)
        import large_scenes

        T = large_scenes.CLASSES[scene]
        return large_scenes.tris(scene), None, tuple(large_scenes.camera_args(T, *LARGE_SCENE_SIZES[scene], shift=d)
                                                     for d in ((0.0, 0.0, 0.0), (0.7, 0.2, 0.4), (-0.5, -0.3, 0.6)))
    if scene == "open5":
        return load_tris("ultracomplex")[0], open5(), _default_cameras()
    if scene == "default":
        return load_tris("default")[0], scene_spheres("default"), _default_cameras()
    return load_tris(scene)[0], None, CUBE_CAMERAS if scene == "cube" else _default_cameras()


@dataclasses.dataclass(frozen=True)
class Case:
    """One enqueue of the matrix.  kind: "rows" (rtc_render_rows_async), "pass" (rtc_render_samples_async: samples
    [first, first + count)) or "first_hit".  cfg: RenderConfig fields beyond the size and spp.  cache: the scene's draw
    cache is on (a few thousand blocks).  must: what has to show a changed byte inside a declared write (scratch regions
    and SCENE_RES names).  prepare: the draw cache's state before the launch -- "reset" (cleared), "same" (filled by this
    launch before) or "moved" (filled from another camera).  cameras: three camera_basis argument lists in place of the
    scene's.  quiet: no byte of the scene's memory may change at all.  rows: (kernel, region or resource name, access) rows the plan is meant to hold -- its intent,
    checked on the CPU.  absent: kernels the plan must not run."""
    name: str
    scene: str
    kind: str = "rows"
    size: tuple = (64, 40)
    spp: int = 2
    cfg: tuple = ()
    segments: bool = False
    first: int = 0
    count: int = 0
    cache: bool = False
    must: tuple = ()
    rows: tuple = ()
    absent: tuple = ()
    prepare: str = ""
    cameras: tuple = ()
    quiet: bool = False

    def camera_args(self):
        return self.cameras or geometry(self.scene)[2]

    def config(self, size=None, **more):
        w, h = size or self.size
        kw = dict(self.cfg)
        sph = geometry(self.scene)[1] is not None
        kw.setdefault("triangles_only", not sph)
        kw.update(more)
        return rt.RenderConfig(w, h, self.spp, 10, **kw)


_CULL = ("mask", "pixMask", "weight")
# (a split launch's tile cull declares the weights written but writes none: they order the one-lane kernel's workgroups)
_SPLIT = ("mask", "pixMask", "geoList", "prim", "geoset")
_SPLIT_ROWS = (("prep", "prim", WRITE), ("tile_cull", "geoList", WRITE), ("tile_cull", "geoset", ATOMIC),
               ("tile_cull", "geoset", WRITE), ("chain", "geoList", READ))
JOINED = [
    Case("split_deferred_cube", "cube", must=_SPLIT + ("samples",),
         rows=_SPLIT_ROWS + (("chain", "samples", WRITE), ("accum", "samples", READ))),
    # (its needles and floor fill the same pixels from each of its cameras: the pixel masks are rewritten as they were)
    Case("split_deferred_layers_33", "layers_33", size=(65, 41), must=("mask", "geoList", "prim", "geoset", "samples"),
         rows=_SPLIT_ROWS + (("chain", "samples", WRITE),)),
    Case("chain_inline", "cube", cfg=(("chain_inline", True),), must=_SPLIT, rows=_SPLIT_ROWS, absent=("accum",)),
    Case("no_coop", "cube", size=(65, 41), cfg=(("coop", False),), must=_CULL + ("order", "prim"),
         rows=(("order", "order", WRITE), ("render", "order", READ)), absent=("chain", "sky")),
    Case("no_tile_cull", "cube", cfg=(("tile_cull", False),), must=("prim",), rows=(("prep", "prim", WRITE),),
         absent=("tile_cull", "chain", "order")),
    Case("segments", "cube", segments=True, must=_SPLIT,
         rows=_SPLIT_ROWS + (("chain", "segslots", ATOMIC), ("reduce", "segslots", WRITE))),
    Case("fsuzane_hits", "fsuzane", size=(65, 41), must=_SPLIT + ("samples",), rows=_SPLIT_ROWS),
    Case("open5_split_spheres", "open5", cfg=(("split_spheres", True),), must=_SPLIT, rows=_SPLIT_ROWS),
    # (the sphere covers the frame from every camera: full pixel masks, equal weights and the same order each time)
    Case("default_sphere_one_lane", "default", must=("mask", "prim"),
         rows=(("order", "order", WRITE), ("render", "order", READ)), absent=("chain", "sky")),
    # 257 mask words and 65 chunks (tests/large_scenes.py): the split launch past one stride of the tile cull's workgroup
    # (the field fills the same pixels from each of its cameras: the pixel masks are rewritten as they were)
    Case("w257_split", "w257", size=LARGE_SCENE_SIZES["w257"], must=("mask", "geoList", "prim", "geoset", "samples"),
         rows=_SPLIT_ROWS + (("chain", "samples", WRITE), ("accum", "samples", READ))),
]
LARGE = [
    Case("super_cull", "cube", size=(1024, 400), spp=1, must=_SPLIT + ("superMask",),
         rows=_SPLIT_ROWS + (("super_cull", "superMask", WRITE), ("tile_cull", "superMask", READ))),
    # (the cube stays within the same superblocks of so wide a frame: their survivor words are rewritten as they were)
    Case("wide_items", "cube", size=(70000, 8), spp=1, must=_SPLIT,
         rows=_SPLIT_ROWS + (("super_cull", "superMask", WRITE),)),
    # 6,145 mask words (tests/large_scenes.py): past the tile cull's cap the launch asks for neither cull nor split launch
    Case("past_cap", "past_cap", size=LARGE_SCENE_SIZES["past_cap"], must=("prim",), rows=(("prep", "prim", WRITE),),
         absent=("tile_cull", "super_cull", "chain", "sky", "order")),
]
# a small row share, pipelined: the planner merges the sky pass behind the geometry kernel
MERGE = Case("merge_small_share", "cube", size=(64, 80), cfg=(("overlap", True), ("row_stride", 2), ("chain_inline", True)),
             must=_SPLIT + ("pixItem", "geoColor"),
             rows=_SPLIT_ROWS + (("tile_cull", "pixItem", WRITE), ("chain", "geoColor", WRITE), ("sky", "geoColor", READ),
                                 ("sky", "pixItem", READ)))
# nine pipelined launches of alternating sizes: every slot (the ninth takes the first one's again) and both cull streams --
# whole frames (every third) keep the caller's stream, the row shares take the cull stream of their slot's parity
OVERLAPPED = [Case(f"overlap_{k}", "cube", size=((64, 40), (65, 82))[k % 3 != 0],
                   cfg=(("overlap", True), ("chain_inline", True)) + ((("row_stride", 2),) if k % 3 else ()),
                   must=("geoList",), rows=_SPLIT_ROWS) for k in range(9)]
CACHED = [Case(f"cached_{what}", "cube", cfg=(("chain_inline", True),), cache=True, must=must, prepare=prepare,
               rows=_SPLIT_ROWS + (("tile_cull", "draw_table", WRITE), ("tile_cull", "item_draw", WRITE),
                                   ("chain", "item_draw", READ)))
          for what, prepare, must in (("cold", "reset", _SPLIT + ("draw_table", "item_draw", "draw_pool")),
                                      ("warm", "same", _SPLIT),
                                      ("camera_step", "moved", _SPLIT + ("draw_table", "item_draw", "draw_pool")))]
PASSES = [
    Case("pass_first", "cube", kind="pass", spp=4, first=0, count=2, must=_SPLIT,
         rows=_SPLIT_ROWS + (("chain", "rng_state", KEYED_WRITE),)),
    Case("pass_later", "cube", kind="pass", spp=4, first=2, count=2, must=_SPLIT,
         rows=_SPLIT_ROWS + (("chain", "rng_state", READ), ("chain", "accum", READ))),
]
FIRST_HIT = [
    # (its tile cull writes no weights: no order kernel follows it)
    Case("first_hit", "cube", kind="first_hit", must=("mask", "pixMask", "prim"),
         rows=(("tile_cull", "mask", WRITE), ("first_hit", "mask", READ), ("first_hit", "hit", WRITE)), absent=("chain", "sky")),
    # no scratch at all (rtc.h); with the slot's primary records current -- the launches before it share its camera origin --
    # no preparation either: nothing of the scene's changes
    Case("first_hit_no_tile_cull", "cube", kind="first_hit", cfg=(("tile_cull", False),), quiet=True,
         cameras=(CUBE_CAMERAS[0],) + tuple((CUBE_CAMERAS[0][0], at, 3.5) for at in ((0.2, -1.5, 0.1), (-0.2, -1.6, 0.0))),
         rows=(("first_hit", "hit", WRITE), ("first_hit", "prim", READ)), absent=("tile_cull", "chain", "sky", "prep")),
]
LAUNCHES = JOINED + LARGE + [MERGE] + OVERLAPPED + CACHED + PASSES + FIRST_HIT
# what the matrix as a whole must show written: every region of the slot and every resource outside it -- but the segment
# slots, which the reduce kernel leaves as it found them (zero): a diff cannot see them written
WHOLE_MATRIX = set(REGIONS) | {"prim", "geoset", "samples", "scene_gen", "draw_table", "item_draw", "membership",
                               "draw_pool"}


# ---- the planner's CPU hooks, for the matrix's intent ----------------------------------------------------------------------
def camera_key(cam):
    return [cam.origin.x, cam.origin.y, cam.origin.z, cam.ex.x, cam.ex.y, cam.ex.z, cam.ey.x, cam.ey.y, cam.ey.z,
            cam.ez.x, cam.ez.y, cam.ez.z, cam.fov]


def env_key(scene):
    v = lambda a: [a.x, a.y, a.z]  # noqa: E731
    return (v(scene.normalizedSunDirection) + v(scene.skyColorHorizon) + v(scene.skyColorZenith) + v(scene.groundColor)
            + [scene.sunFocus, scene.sunIntensity])


class Sim:
    """One rtc_plan_sim handle shaped like a scene of the matrix."""

    IDS = dict(colors=0x1000, accum=0x2000, rng=0x3000, hit=(0x4000, 0x5000, 0x6000, 0x7000))

    def __init__(self, scene, cache=False, tri_count=None):
        """tri_count: a scene of that many triangles and no sphere, in place of the named one's."""
        tris, sph, _ = geometry(scene) if tri_count is None else (None, None, None)
        self.L = rt.lib()
        self.h = C.c_void_p()
        assert self.L.rtc_plan_sim_create(len(tris) if tri_count is None else tri_count, 0, C.byref(self.h)) == 0
        if sph is not None:  # (the matrix's sphere scenes: `default` stays on the one-lane kernel, open5 is forced)
            assert self.L.rtc_plan_sim_set_spheres(self.h, len(sph), 0) == 0
        assert self.L.rtc_plan_sim_set_draw_cache(self.h, int(cache)) == 0
        self.ops = (C.c_int * (4 * 64))()
        self.fp = (C.c_ulonglong * (6 * 256))()

    def close(self):
        self.L.rtc_plan_sim_release(self.h)

    def _decode(self, rc):
        assert rc > 0, rc
        ops = np.frombuffer(self.ops, np.int32, 4 * (rc & 0xff)).reshape(-1, 4).copy()
        rows = np.frombuffer(self.fp, np.uint64, 6 * (rc >> 8)).reshape(-1, 6).copy()
        return split_plan(ops, rows)

    def launch(self, case, cam_args, size=None, **more):
        d = case.config(size, **more).desc()
        if case.kind == "first_hit":
            d.flags = d.flags & rt.RTC_F_NO_TILE_CULL
            assert self.L.rtc_plan_sim_set_first_hit(self.h, *self.IDS["hit"]) == 0
        if case.kind == "pass":
            assert self.L.rtc_plan_sim_set_sample_range(self.h, case.first, case.count, self.IDS["rng"]) == 0
        cam = (C.c_float * 13)(*camera_key(rt.camera_basis(*cam_args)))
        env = (C.c_float * 14)(*env_key(rt.default_scene()))
        rc = self.L.rtc_plan_sim_launch(self.h, C.byref(d), 0, self.IDS["colors"], self.IDS["accum"], int(case.segments),
                                        cam, env, self.ops, 64, self.fp, 256)
        return self._decode(rc)

    def regions(self):
        """{region name: (lo, hi)} of the last launch's bound scratch regions (absolute offsets in the scratch)."""
        out = (C.c_ulonglong * (3 * 16))()
        n = self.L.rtc_plan_sim_regions(self.h, out, 16)
        assert n >= 2
        return {REGIONS[int(out[3 * r])]: (int(out[3 * r + 1]), int(out[3 * r + 1]) + int(out[3 * r + 2]))
                for r in range(2, n)}


def named_rows(ops, plan_rows, regions=None):
    """{(kernel name, region or resource name, access)} of a plan; scratch rows are named through `regions` ({name: (lo,
    hi)}, Sim.regions) where given, else as "scratch"."""
    by_range = {v: k for k, v in (regions or {}).items()}
    out = set()
    for row in plan_rows:
        i, res, access, _, lo, hi = (int(v) for v in row)
        name = by_range.get((lo, hi), "scratch") if res == RES_SCRATCH else RES_NAMES[res]
        out.add((KNAMES[int(ops[i][3])], name, access))
    return out


def kernels_of(ops):
    return [KNAMES[int(o[3])] for o in ops if int(o[0]) == 0]
