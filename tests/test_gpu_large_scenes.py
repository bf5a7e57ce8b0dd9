"""The scenes of tests/large_scenes.py -- 16,385, 393,216 and 393,217 triangles: 257, 6,144 and 6,145 mask words, 65, 1,536
and 1,537 chunks -- on every route of the renderer and in every query, against the CPU oracle: floats as bits, NaN
positions, u8 frames, segment counts, no tolerance.  tests/test_large_scenes.py shows without a GPU that the frames and
the ray sets reach both ends of the mask words (the reference order) and of the chunks (the cluster order).

One DeviceScene per class serves the whole module; the oracle's results are computed once and are read-only.  Besides the
values, every frame test asserts the route its launch took (DeviceScene.last_plan, chain_report): w257 and cap run the
tile cull and rtc_render_chain over more than one chunk (MULTI), past_cap runs neither.  No launch here takes the draw
cache: a launch is eligible for it only where the scene is one chunk (draw_cache_eligible, rtc_render.hip), so at 65 chunks
and more the routes with and without RTC_F_NO_DRAW_CACHE are the same launch -- both are run, as both must give the
oracle's frame, and after every frame the cache must hold no block at any of the three sizes."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import footprints as fpt
import large_scenes as ls
import moving_scenes
import occlusion_reference as ocr
import oracle.binding as orc
import pixel_pass_reference as ppr
import progressive_reference as pr
import raytracingc_amd as rt
import test_gpu_cluster
import test_gpu_primary_cull
import trace_paths_reference as tpr
import trace_rays_reference as tr
from test_gpu_scene_update import _assert_records

pytestmark = pytest.mark.gpu

NAMES = sorted(ls.CLASSES)
CULLED = ("w257", "cap")  # the classes at or below the tile cull's cap
ZERO = dict.fromkeys(tr.NAMES, 0)
NO_CULL, WAVE = rt.RTC_F_NO_CLUSTER_CULL, rt.RTC_F_WAVE_PER_RAY
HALF_BAND = dict(row_start=0, row_stride=2, row_band=8)
HALF_ROWS = dict(row_start=1, row_stride=2)
ROUTES = {
    "joined": dict(), "no_tile_cull": dict(tile_cull=False), "no_coop": dict(coop=False), "inline": dict(chain_inline=True),
    "hoisted": dict(hoist=True), "no_cluster_cull": dict(cluster_cull=False), "segments": dict(),
    "half_band": dict(overlap=True, **HALF_BAND), "half_band_no_cache": dict(overlap=True, draw_cache=False, **HALF_BAND),
    "half_rows": dict(overlap=True, **HALF_ROWS), "half_rows_no_cache": dict(overlap=True, draw_cache=False, **HALF_ROWS),
}
PATH_SPP, PATH_BOUNCE = 3, 10
# every k-th query ray traces paths.  At the two cap sizes the CPU reference of all 1,783 rays takes 22.8 s against 6.3 s for
# every fourth (profiles/r37_durations.txt): the full set would make this the suite's slowest test.  The ray set is thinned,
# never the triangle count; trace_rays and occluded run every ray.
PATH_EVERY = {"w257": 1, "cap": 4, "past_cap": 4}


@pytest.fixture(scope="module")
def scenes(gpu_available):
    """name -> the class's DeviceScene, uploaded at its first use and never again."""
    held = {}

    def get(name):
        if name not in held:
            held[name] = rt.DeviceScene(ls.tris(name), None)
        return held[name]

    yield get
    import torch

    torch.cuda.synchronize()
    for ds in held.values():
        ds.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(rays):
    import torch

    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6).copy()).cuda()


def _compare(what, col, a, ocol, oacc):
    nan = np.isnan(oacc)
    assert np.array_equal(np.isnan(a), nan), f"{what}: NaN positions differ ({int(np.isnan(a).sum())} vs {int(nan.sum())})"
    bad = int(((_bits(a) != _bits(oacc)) & ~nan).any(-1).sum())
    assert bad == 0, f"{what}: {bad} pixels' accumulator bits differ"
    assert np.array_equal(col, ocol), f"{what}: {int((col != ocol).any(-1).sum())} u8 pixels differ"


def _render(ds, cam, cfg, counters=False):
    """(u8, floats, segments or None, kernels of the plan, chain_report before, after) of one launch, complete."""
    import torch

    rows = cfg.rows()
    out = torch.zeros((rows, cfg.width, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((rows, cfg.width, 3), dtype=torch.float32, device="cuda")
    seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
    torch.cuda.synchronize()
    before = ds.chain_report()
    ds.render_rows_async(rt.default_scene(), cam, cfg, out.data_ptr(), acc.data_ptr(), seg.data_ptr() if counters else None,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    kernels = fpt.kernels_of(fpt.split_plan(*ds.last_plan())[0])
    return (out.cpu().numpy(), acc.cpu().numpy(), int(seg.cpu().numpy()[0]) if counters else None, kernels, before,
            ds.chain_report())


def _assert_route(name, route, counters, kernels, before, after, what):
    """The launch ran what its class and route mean it to run."""
    _, _, clusters, chunks = ls.counts(ls.CLASSES[name])
    cull = name in CULLED and route != "no_tile_cull"
    chain = cull and route != "no_coop"
    assert ("tile_cull" in kernels) == cull, f"{what}: {kernels}"
    assert ("chain" in kernels) == chain and ("sky" in kernels) == chain, f"{what}: {kernels}"
    assert ("render" in kernels) == (not chain), f"{what}: {kernels}"
    assert ("reduce" in kernels) == counters, f"{what}: {kernels}"
    if chain:
        assert after["launches"] == before["launches"] + 1, what
        assert after["multi"] and after["general"] and after["count"] == counters, f"{what}: {after}"
        assert (after["cluster_count"], after["chunk_count"]) == (clusters, chunks), f"{what}: {after}"
    else:
        assert after == before, f"{what}: a geometry-kernel launch"


# ---- frames on every route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", NAMES)
def test_frame_matches_oracle(name, route, scenes):
    kw = ROUTES[route]
    share = {k: kw[k] for k in ("row_start", "row_stride", "row_band") if k in kw}
    ocol, oacc, oseg = ls.frame_oracle(name, **share)
    ds, counters = scenes(name), route == "segments"
    what = f"{name} {route}"
    col, acc, seg, kernels, before, after = _render(ds, ls.frame_camera(name), ls.frame_config(name, **kw), counters)
    _assert_route(name, route, counters, kernels, before, after, what)
    _compare(what, col, acc, ocol, oacc)
    if counters:
        assert seg == oseg, f"{what}: segments {seg} vs {oseg}"
    st = ds.draw_cache_stats()  # (more than one chunk, or no split launch at all: nothing takes a block of the draw cache)
    assert st["blocks"] == 0 and st["fresh"] == 0, f"{what}: {st}"


# ---- first hit -------------------------------------------------------------------------------------------------------------
def _flat(bufs):
    return {k: v.reshape(-1, 3) if k in ("normal", "albedo") else v.reshape(-1) for k, v in bufs.items()}


@pytest.mark.parametrize("tile_cull", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_first_hit_matches_oracle(name, tile_cull, scenes):
    ds = scenes(name)
    got = _flat(ds.first_hit(ls.frame_camera(name), ls.frame_config(name, tile_cull=tile_cull)))
    kernels = fpt.kernels_of(fpt.split_plan(*ds.last_plan())[0])
    assert ("tile_cull" in kernels) == (tile_cull and name in CULLED) and kernels[-1] == "first_hit", kernels
    bad = tr.differing(got, ls.expected(name, "frame"))
    print(f"first hit {name} tile_cull={tile_cull}: differing {bad}")
    assert set(got) == set(tr.NAMES) and bad == ZERO


# ---- queries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, NO_CULL])
@pytest.mark.parametrize("name", NAMES)
def test_trace_rays(name, flags, scenes):
    ds, rays, want = scenes(name), ls.query_rays(name), ls.expected(name, "rays")
    d = _dev(rays)
    assert tr.differing(ds.trace_rays(d, True, tr.NAMES, flags), want) == ZERO, f"{name} flags {flags:#x}"
    if name == "w257":
        order = ds.ray_order(d)
        assert sorted(order.cpu().numpy().tolist()) == list(range(len(rays)))
        assert tr.differing(ds.trace_rays(d, True, tr.NAMES, flags, order=order), want) == ZERO, f"{name} ordered"


@pytest.mark.parametrize("limit", ["none", "median"])
@pytest.mark.parametrize("name", NAMES)
def test_occluded(name, limit, scenes):
    ds, rays, e = scenes(name), ls.query_rays(name), ls.expected(name, "rays")
    lim = ocr.limits(limit, e["prim"], e["depth"])
    with np.errstate(all="ignore"):
        want = (e["prim"] != -1) & (e["depth"].astype(np.float32) < ocr._f32(lim, len(rays)))
    assert want.any() and not want.all()
    if limit == "median":
        assert (want != (e["prim"] != -1)).sum() >= 100, "the limit must decide"
    d = _dev(rays)
    for flags in (0, NO_CULL):
        got, count = ds.occluded(d, lim, True, flags, count=True)
        assert np.array_equal(got, want) and count == int(want.sum()), f"{name} {limit} flags {flags:#x}"
    if name == "w257":
        got, count = ds.occluded(d, lim, True, 0, count=True, order=ds.ray_order(d))
        assert np.array_equal(got, want) and count == int(want.sum()), f"{name} {limit} ordered"


@functools.lru_cache(maxsize=None)
def _path_set(name):
    rays = np.ascontiguousarray(ls.query_rays(name)[::PATH_EVERY[name]])
    seeds = tpr.hash_seeds(len(rays))
    want = tpr.expected(ls.tris(name), None, rt.default_scene(), 1, rays, seeds, PATH_SPP, PATH_BOUNCE)
    rays.setflags(write=False)
    return rays, seeds, want


@pytest.mark.parametrize("kernel", ["lane", "wave"])
@pytest.mark.parametrize("name", NAMES)
def test_trace_paths(name, kernel, scenes):
    import torch

    rays, seeds, (radiance, states, segments) = _path_set(name)
    assert segments > 2 * len(rays), "the paths bounce"
    ds, d = scenes(name), _dev(rays)
    sd = torch.from_numpy(seeds.view(np.int32).copy()).cuda()
    orders = [None] + ([ds.ray_order(d)] if name == "w257" else [])
    for order in orders:
        got = ds.trace_paths(d, sd, rt.default_scene(), PATH_SPP, PATH_BOUNCE, True, WAVE if kernel == "wave" else 0,
                             segments=True, order=order)
        what = f"{name} {kernel} order={order is not None}"
        assert tpr.differing(got["radiance"], radiance) == 0, what
        assert tpr.differing(got["seeds"], states) == 0 and got["segments"] == segments, what


# ---- moving geometry -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _moved(name, helper):
    out = moving_scenes.HELPERS[helper](ls.tris(name))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _moved_oracle(name, helper):
    """The oracle's (u8, floats) of the class's frame and its first-hit buffers on the moved triangles."""
    moved = _moved(name, helper)
    ocol, oacc, _ = orc.render(moved, None, rt.default_scene(), ls.frame_camera(name), ls.frame_config(name).desc(), threads=16)
    ocol.setflags(write=False)
    oacc.setflags(write=False)
    assert (_bits(oacc) != _bits(ls.frame_oracle(name)[1])).any(-1).sum() > 20, "the move must show"
    return ocol, oacc, tr.expected(moved, None, 1, ls.launch_primary(name, "frame"))


def _frame_and_first_hit(ds, name, helper, what):
    """A frame and a first-hit launch of the class against the oracle on the moved triangles."""
    cfg, cam = ls.frame_config(name), ls.frame_camera(name)
    ocol, oacc, want = _moved_oracle(name, helper)
    col, acc, _, kernels, _, after = _render(ds, cam, cfg)
    assert "tile_cull" in kernels and "chain" in kernels and after["multi"]
    _compare(what, col, acc, ocol, oacc)
    assert tr.differing(_flat(ds.first_hit(cam, cfg)), want) == ZERO, f"{what}: first hit"


@pytest.mark.parametrize("helper", ["shift", "squash"])
def test_w257_update_then_regroup(helper, gpu_available):
    """update(moved): the records are the upload's grouping refitted (scene_records_host(tris, moved)) and the launches
    the oracle's on the moved triangles; update(moved, regroup=True): the records are a fresh upload's of them."""
    name = "w257"
    tris, moved = ls.tris(name), _moved(name, helper)
    ds = rt.DeviceScene(tris, None)
    try:
        ds.update(moved)
        _assert_records(ds.records(), rt.scene_records_host(tris, moved), f"{name} {helper} updated")
        _frame_and_first_hit(ds, name, helper, f"{name} {helper} updated")
        ds.update(moved, regroup=True)
        fresh = rt.scene_records_host(moved)
        assert np.array_equal(rt.regroup_membership_host(moved), fresh["clTris"][:len(moved), 12].view(np.int32))
        _assert_records(ds.records(), fresh, f"{name} {helper} regrouped")
        _frame_and_first_hit(ds, name, helper, f"{name} {helper} regrouped")
    finally:
        ds.close()


def test_cap_update_refits_1536_chunks(scenes):
    """One shift of the cap scene (rtc_refit runs one workgroup per chunk) and a first-hit launch; then back."""
    name = "cap"
    ds, moved = scenes(name), _moved(name, "shift")
    cfg, cam = ls.frame_config(name), ls.frame_camera(name)
    want = tr.expected(moved, None, 1, ls.launch_primary(name, "frame"))
    assert tr.differing(want, ls.expected(name, "frame"))["depth"] > 20, "the move must show"
    try:
        ds.update(moved)
        for tile_cull in (True, False):
            got = _flat(ds.first_hit(cam, ls.frame_config(name, tile_cull=tile_cull)))
            assert tr.differing(got, want) == ZERO, f"cap shifted, tile_cull={tile_cull}"
    finally:
        ds.update(ls.tris(name))
    assert tr.differing(_flat(ds.first_hit(cam, cfg)), ls.expected(name, "frame")) == ZERO, "cap moved back"


# ---- progressive passes and pixel passes, w257 -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pass_reference():
    name = "w257"
    d, cache = ls.frame_config(name).desc(), {}
    args = (ls.tris(name), None, rt.default_scene(), ls.frame_camera(name), d)
    chain = pr.chain(*args, [2, 1], cache)
    states = ppr.per_sample(*args, cache)
    classes = ppr.classes(pr.hits_per_sample(*args, cache))
    return chain, states, classes


def test_w257_two_passes_equal_the_single_launch(scenes):
    name = "w257"
    ds, cfg = scenes(name), ls.frame_config(name)
    chain = _pass_reference()[0]
    ocol, oacc, _ = ls.frame_oracle(name)
    got = list(ds.render_progressive(rt.default_scene(), ls.frame_camera(name), cfg, [2, 1]))
    for (done, col, acc), (rdone, racc, rrng, rcol, _) in zip(got, chain):
        assert done == rdone
        _compare(f"{name} after {done} samples", col, acc, rcol.reshape(col.shape), racc.reshape(acc.shape))
    _compare(f"{name} 2 + 1 samples against the single launch", got[-1][1], got[-1][2], ocol, oacc)
    assert np.array_equal(ds.progress.rng.reshape(-1), chain[-1][2].reshape(-1))


@pytest.mark.parametrize("kernel", ["lane", "wave"])
def test_w257_pixel_pass(kernel, scenes):
    """A whole pass [0, 2), then a pass [2, 3) over 64 listed pixels -- pixels that hit several times, once and never, and
    one index past the frame -- against tests/pixel_pass_reference.py: the listed pixels move on, every other byte stays."""
    import torch

    name = "w257"
    ds, cfg, cam, scene = scenes(name), ls.frame_config(name), ls.frame_camera(name), rt.default_scene()
    _, states, classes = _pass_reference()
    n = cfg.width * cfg.height
    listed = np.concatenate([ppr.mixed_list(classes, 63), np.array([n + 5], np.uint32)])
    assert all(c > 0 for c in ppr.class_counts(classes, listed[:-1])), "geometry and sky are both listed"
    ref = ppr.Frame(states, fill=0)
    ref.whole_pass(0, 2)
    calls = ref.pixel_pass(2, 1, listed)
    col = torch.zeros((cfg.height, cfg.width, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((cfg.height, cfg.width, 3), dtype=torch.float32, device="cuda")
    rng = torch.zeros((cfg.height, cfg.width), dtype=torch.int32, device="cuda")
    ds.render_samples_async(scene, cam, cfg, 0, 2, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    px = torch.from_numpy(listed.view(np.int32).copy()).cuda()
    res = ds.render_pixels(scene, cam, cfg, 2, 1, px, acc, rng, col, segments=True, flags=WAVE if kernel == "wave" else 0)
    torch.cuda.synchronize()
    wacc, wrng, wcol = ref.buffers()
    assert int((acc.cpu().numpy().view(np.uint32).reshape(n, 3) != wacc).sum()) == 0, "accumulator words"
    assert int((rng.cpu().numpy().view(np.uint32).reshape(n) != wrng).sum()) == 0, "RNG states"
    assert int((col.cpu().numpy().reshape(n, 3) != wcol).sum()) == 0, "Color bytes"
    assert res["segments"] == calls


# ---- the proofs at scale, w257 ---------------------------------------------------------------------------------------------
def test_w257_primary_cull_is_sound(gpu_available, monkeypatch):
    """tests/test_gpu_primary_cull.py's checks, unchanged, on 561 pixels x 16,385 triangles = 9.2 M pairs: no hit is filtered
    out per pixel, per tile or in the pixel mask, over 257 mask words."""
    name = "w257"
    cam = ls.camera(ls.CLASSES[name], 33, 17)
    monkeypatch.setitem(test_gpu_primary_cull.SCENES, name, (ls.tris(name), cam, "large field; filter active"))
    p = test_gpu_primary_cull._check(name, rt.RenderConfig(33, 17, 1, 4, True))
    assert p["words"] == 257
    assert (p["tile_bits"][:, 256] & np.uint64(1)).any(), "some tile keeps the awning, bit 0 of word 256"


def test_w257_cluster_bounds_are_sound(gpu_available):
    """tests/test_gpu_cluster.py's rays and assertions on 2,049 cluster balls and 65 chunk balls."""
    tris = ls.tris("w257")
    rays = test_gpu_cluster._rays(tris, 40_000, np.random.default_rng(1234 + 257))
    r = rt.cluster_bound_probe(tris, rays)
    print("w257", r)
    assert r["violations"] == 0 and r["reach_violations"] == 0, r
    assert r["hits"] > 1_000 and r["unreachable"] > 0
    assert r["culled"] > r["tests"] // 8  # the bound is not vacuous
