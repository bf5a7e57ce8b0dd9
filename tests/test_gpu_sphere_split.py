"""Sphere scenes through the split launch: rtc_tile_cull's sphere coverage, the sky pass and
rtc_render_chain<SPHERES> against the CPU oracle (calculateRayCollision's sphere loop first, raytracing.c:219-228, then
the triangles; raySphere raytracing.c:162-184).  Every frame is compared bit for bit -- accumulator float bits, the u8
frame and the segment count -- on three routes: forced split (RTC_F_SPLIT_SPHERES), the one-lane-per-pixel kernel
(coop=False) and the upload gate's default routing."""
from __future__ import annotations

import dataclasses
import functools
import hashlib

import numpy as np
import pytest

from conftest import load_tris, render_golden, scene_spheres, setup_from_flags
from env_edge_scenes import primary_rays
from sphere_scenes import closing_sphere, open5, open5_padded, tie_scene

import oracle.binding as orc
import raytracingc_amd as rt
from raytracingc_amd._abi import RtcRenderDesc
from raytracingc_amd.distributed import band_rows, rank_config, rows_per_rank

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _geometry(name):
    """(triangles, spheres, Scene, camera) of a test scene."""
    scene, cam, _ = setup_from_flags({})
    if name == "open5":
        return load_tris("ultracomplex")[0], open5(), scene, cam
    if name == "tie":
        t, s = tie_scene()
        return t, s, scene, rt.camera_basis((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 1.0)
    if name == "default":
        return load_tris("default")[0], scene_spheres("default"), scene, cam
    if name == "spheres_only":
        return None, open5(), scene, cam
    if name == "multi_chunk":
        return load_tris("suzannes")[0], open5(), scene, cam
    if name == "inside":
        return load_tris("cube")[0], closing_sphere(50.0), scene, cam
    if name == "open5_32":
        return load_tris("ultracomplex")[0], open5_padded(32), scene, cam
    if name == "open5_33":
        return load_tris("ultracomplex")[0], open5_padded(33), scene, cam
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle(name, W, H, spp, mb=10, tonly=0, flags=0):
    """The oracle's (u8 frame, accumulator, segments), computed once per configuration and shared (read-only)."""
    tris, sph, scene, cam = _geometry(name)
    col, acc, seg = orc.render(tris, sph, scene, cam, RtcRenderDesc(W, H, spp, mb, tonly, 0, 1, flags), threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


@functools.lru_cache(maxsize=None)
def _device_scene(name):
    tris, sph, _, _ = _geometry(name)
    return rt.DeviceScene(tris, sph)


def _launch(name, cfg, counters=False):
    """One joined launch on the scene's DeviceScene -> (u8, accumulator, segment counters or None)."""
    import torch

    _, _, scene, cam = _geometry(name)
    ds = _device_scene(name)
    rows = cfg.rows()
    out = torch.zeros((rows, cfg.width, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((rows, cfg.width, 3), dtype=torch.float32, device="cuda")
    seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
    st = torch.cuda.current_stream().cuda_stream
    ds.render_rows_async(scene, cam, cfg, out.data_ptr(), acc.data_ptr(), seg.data_ptr() if counters else None, st)
    torch.cuda.synchronize()
    return out.cpu().numpy(), acc.cpu().numpy(), (seg.cpu().numpy() if counters else None)


def _check(name, cfg, what, counters=True):
    ocol, oacc, oseg = _oracle(name, cfg.width, cfg.height, cfg.spp, cfg.max_bounce, int(cfg.triangles_only))
    col, acc, seg = _launch(name, cfg, counters)
    assert np.array_equal(col, ocol), f"{name} {what}: {int((col != ocol).any(-1).sum())} u8 pixels differ"
    if cfg.height // 2 == 0:  # every direction NaN (main.c:88-89): the NaN sign differs between x86 and gfx950
        assert np.isnan(acc).all() and np.isnan(oacc).all()
    else:
        bad = int((_bits(acc) != _bits(oacc)).any(-1).sum())
        assert bad == 0, f"{name} {what}: {bad} pixels' accumulator bits differ"
    if counters:
        assert int(seg[0]) == oseg, f"{name} {what}: segments {int(seg[0])} vs the oracle's {oseg}"
    return acc


def _cfg(W, H, spp, mb=10, **kw):
    return rt.RenderConfig(W, H, spp, mb, kw.pop("triangles_only", False), **kw)


# ---- 1. the path taken ----------------------------------------------------------------------------------------
def test_path_taken(gpu_available):
    """kernel_times() reports the split launch's two kernels only when a launch took it: a forced sphere launch does,
    coop=False and 33 spheres do not."""
    ds = _device_scene("open5")
    assert isinstance(ds.sphere_split, bool)
    ds.set_timing(True)
    try:
        _launch("open5", _cfg(96, 54, 8, split_spheres=True))
        kt = ds.kernel_times()
        assert kt is not None and kt[0] > 0 and kt[1] > 0
        _launch("open5", _cfg(96, 54, 8, split_spheres=True, coop=False))
        assert ds.kernel_times() is None
    finally:
        ds.set_timing(False)
    ds33 = _device_scene("open5_33")
    assert ds33.sphere_split is False
    ds33.set_timing(True)
    try:
        _launch("open5_33", _cfg(96, 54, 4, split_spheres=True))
        assert ds33.kernel_times() is None
    finally:
        ds33.set_timing(False)
    # the gate's decisions: the open scene takes the split launch; the closed box and a scene of spheres alone stay on
    # the pixel kernel; no spheres, no decision
    assert ds.sphere_split is True and _device_scene("multi_chunk").sphere_split is True
    assert _device_scene("default").sphere_split is False and _device_scene("spheres_only").sphere_split is False
    ds.set_timing(True)
    try:
        _launch("open5", _cfg(96, 54, 8))  # default routing: the gate sends it to the split launch
        assert ds.kernel_times() is not None
    finally:
        ds.set_timing(False)
    tri_only = rt.DeviceScene(load_tris("cube")[0], None)
    assert tri_only.sphere_split is False
    tri_only.close()


# ---- the test scene is not vacuous ------------------------------------------------------------------------------
def test_open5_covers_every_case(gpu_available):
    """The conditions that keep the open5 tests from passing vacuously, on the oracle at 96x54.  From debug-bounce
    renders of the parts (maxBounce 1: a pixel is white where its primary ray hits the part): each of spheres 0-3 covers
    >= 10 pixels (24, 13, 11, 1822), sphere 4 (behind the camera) none, the triangles >= 100 (192), and at least half the
    frame is sky (3234 of 5184).  Resolved by depth with the oracle's own raySphere / rayTriangle, spheres 2 and 3 and the
    triangles are the closest hit of 11, 1770 and 169 pixels; spheres 0 and 1 lie behind the model in this view (every
    pixel they cover has a closer triangle), so they are reached by bounce rays only -- the mirror ball and the glossy
    one still decide those samples."""
    W, H = 96, 54
    tris, sph, scene, cam = _geometry("open5")

    def part(t, s):
        d = RtcRenderDesc(W, H, 1, 1, int(s is None), 0, 1, rt.RTC_F_DEBUG_BOUNCES)
        return int((orc.render(t, s, scene, cam, d, threads=8)[0] == 255).all(-1).sum())

    parts = [part(None, sph[i:i + 1]) for i in range(len(sph))] + [part(tris, None)]
    print(f"open5 96x54 coverage of the parts: spheres {parts[:5]}, triangles {parts[5]}")
    assert all(c >= 10 for c in parts[:4]) and parts[4] == 0 and parts[5] >= 100
    rays = primary_rays(cam, W, H)
    n = len(rays)
    best = np.full(n, 999999.0, np.float32)
    owner = np.full(n, -1)
    for i in range(len(sph)):  # spheres first, in index order, strictly closer (raytracing.c:219-228)
        hit, dst, _ = orc.ray_sphere(rays, np.repeat(sph[i:i + 1], n))
        win = (hit != 0) & (dst < best)
        best[win], owner[win] = dst[win], i
    for t in range(len(tris)):
        hit, dst = orc.ray_triangle(rays, np.repeat(tris[t:t + 1], n))
        win = (hit != 0) & (dst < best)
        best[win], owner[win] = dst[win], len(sph)
    counts = [int((owner == i).sum()) for i in range(len(sph) + 1)]
    sky = int((owner < 0).sum())
    print(f"open5 96x54 primary hits: spheres {counts[:5]}, triangles {counts[5]}, sky {sky} of {n}")
    assert counts[2] >= 10 and counts[3] >= 10 and counts[4] == 0 and counts[5] >= 100 and 2 * sky >= n
    dbg, _, _ = _oracle("open5", W, H, 1, 1, 0, rt.RTC_F_DEBUG_BOUNCES)
    assert np.array_equal((dbg.reshape(-1, 3) == 255).all(-1), owner >= 0)
    _, _, seg = _oracle("open5", W, H, 8)
    assert 1.0 < seg / (W * H * 8) < 2.0  # an open scene: most bounce rays escape (1.22 segments per sample)


def test_tie_scene_keeps_the_first_sphere(gpu_available):
    """Equal distances: along the centre ray the two spheres and the triangle are all at exactly 4.0f; the reference
    keeps sphere 0 (red) -- spheres before triangles, lowest index, strict <.  Its neighbours see the triangle (green)."""
    ocol, oacc, _ = _oracle("tie", 8, 8, 1, 1)
    assert oacc[4, 4].tolist() == [1.0, 0.0, 0.0]
    for y, x in [(4, 3), (4, 5), (3, 4), (5, 4)]:
        assert oacc[y, x].tolist() == [0.0, 1.0, 0.0], (y, x)
    _check("tie", _cfg(8, 8, 1, 1, split_spheres=True), "forced split")


# ---- 2 / 3. bit-exact on three routes ----------------------------------------------------------------------------
CASES = [("open5", 96, 54, 8, 10), ("tie", 8, 8, 1, 1), ("default", 64, 36, 4, 10), ("default", 160, 90, 4, 10),
         ("spheres_only", 64, 36, 4, 10), ("multi_chunk", 64, 48, 2, 10), ("inside", 64, 36, 4, 10),
         ("open5_32", 96, 54, 4, 10), ("open5_33", 96, 54, 4, 10)]
ROUTES = {"split": dict(split_spheres=True), "nocoop": dict(coop=False), "auto": {}}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name,W,H,spp,mb", CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}x{c[3]}" for c in CASES])
def test_routes_bit_exact(name, W, H, spp, mb, route, gpu_available):
    """Every scene on every route equals the oracle (so the three routes' frames are identical), with the segment
    counters (the counting instantiations) and without them (the plain ones)."""
    cfg = _cfg(W, H, spp, mb, **ROUTES[route])
    acc = _check(name, cfg, route, counters=True)
    acc2 = _check(name, cfg, route + " (no counters)", counters=False)
    assert np.array_equal(_bits(acc), _bits(acc2)) or H // 2 == 0
    if (name, W) == ("default", 160):  # the reference binary's own frame (tests/golden/make_golden.py)
        assert hashlib.sha256(acc.tobytes()).hexdigest() == render_golden()["default_160x90x4"]["float_sha256"]


# ---- 4. variants on open5 ---------------------------------------------------------------------------------------
VARIANTS = {"hoist": (96, 54, 8, 10, dict(hoist=True)), "chain_inline": (96, 54, 8, 10, dict(chain_inline=True)),
            "hoist_inline": (96, 54, 8, 10, dict(hoist=True, chain_inline=True)),
            "spp70": (48, 27, 70, 10, {}), "spp70_hoist": (48, 27, 70, 10, dict(hoist=True)),
            "spp1": (96, 54, 1, 10, {}), "bounce1": (96, 54, 8, 1, {}),
            "bounce0": (96, 54, 8, 0, {}), "nan_7x1": (7, 1, 3, 10, {}), "odd_121x67": (121, 67, 4, 10, {}),
            "no_cluster_cull": (96, 54, 8, 10, dict(cluster_cull=False))}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_open5_variants(variant, gpu_available):
    W, H, spp, mb, kw = VARIANTS[variant]
    for counters in (True, False):
        _check("open5", _cfg(W, H, spp, mb, split_spheres=True, **kw), variant, counters)


def test_triangles_only_on_a_sphere_scene(gpu_available):
    """trianglesOnly (main.c:113, :241) on a scene uploaded with spheres renders none of them: the triangle-only frame."""
    cfg = _cfg(96, 54, 8, triangles_only=True, split_spheres=True)
    acc = _check("open5", cfg, "triangles only")
    tris, _, scene, cam = _geometry("open5")
    _, ref, _ = rt.render(tris, None, scene, cam, cfg, want_accum=True)
    assert np.array_equal(_bits(acc), _bits(ref))
    assert not np.array_equal(_bits(acc), _bits(_oracle("open5", 96, 54, 8)[1]))  # (the spheres do show otherwise)


# ---- 5. row shares ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [1, 8])
@pytest.mark.parametrize("overlap", [False, True])
def test_row_shares_assemble(overlap, band, gpu_available):
    """G = 8 ranks' shares (single rows or bands of 8), each rendered on this device by the forced split -- small shares
    sum in-kernel and, pipelined, run the merged sky pass on the alternating streams -- assemble to the whole frame."""
    import torch

    W, H, spp, G = 160, 96, 8, 8
    ocol, oacc, _ = _oracle("open5", W, H, spp)
    _, _, scene, cam = _geometry("open5")
    ds = _device_scene("open5")
    st = torch.cuda.current_stream().cuda_stream
    rows = rows_per_rank(H, G, band)
    out = torch.zeros((G, rows, W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((G, rows, W, 3), dtype=torch.float32, device="cuda")
    for r in range(G):
        cfg = rank_config(_cfg(W, H, spp, overlap=overlap, split_spheres=True), r, G, band)
        ds.render_rows_async(scene, cam, cfg, out[r].data_ptr(), acc[r].data_ptr(), None, st)
    torch.cuda.synchronize()
    o, a = out.cpu().numpy(), acc.cpu().numpy()
    for r in range(G):
        ys = np.asarray(band_rows(H, r, G, band))
        assert np.array_equal(o[r, :len(ys)], ocol[ys]), f"rank {r} bytes"
        assert np.array_equal(_bits(a[r, :len(ys)]), _bits(oacc[ys])), f"rank {r} floats"


# ---- 6. pipelined frames --------------------------------------------------------------------------------------------
def test_frame_loop_pipelined(gpu_available):
    import torch

    W, H, spp = 256, 144, 8
    ocol, _, _ = _oracle("open5", W, H, spp)
    _, _, scene, cam = _geometry("open5")
    ds = _device_scene("open5")
    st = torch.cuda.Stream()
    dev = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    host = [torch.zeros((H, W, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    seen = []
    for frames in (3, 4):  # the last writer of buffer 0 is frame 2, then of both buffers frames 2 and 3
        out = ds.frame_loop(scene, cam, _cfg(W, H, spp, split_spheres=True), [d.data_ptr() for d in dev],
                            [h.data_ptr() for h in host], W * 3, frames, st.cuda_stream)
        assert out["frames"] == frames
        seen.append([np.array_equal(h.numpy(), ocol) for h in host])
    assert seen == [[True, True], [True, True]]


# ---- 7. sphere and triangle-only launches mixed on one scene ------------------------------------------------------
def test_mixed_launches_overlapped(gpu_available):
    import torch

    W, H, spp = 160, 96, 8
    with_s, _, _ = _oracle("open5", W, H, spp)
    without, _, _ = _oracle("open5", W, H, spp, 10, 1)
    _, _, scene, cam = _geometry("open5")
    ds = _device_scene("open5")
    st = torch.cuda.Stream()
    out = torch.zeros((6, H, W, 3), dtype=torch.uint8, device="cuda")
    last = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k in range(6):
        cfg = _cfg(W, H, spp, overlap=True, split_spheres=True, triangles_only=bool(k & 1))
        ds.render_rows_async(scene, cam, cfg, out[k].data_ptr(), stream=st.cuda_stream)
    # a joined launch waits for every pending sky pass before its first kernel and joins its own
    ds.render_rows_async(scene, cam, _cfg(W, H, spp, split_spheres=True), last.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    for k in range(6):
        assert np.array_equal(o[k], without if k & 1 else with_s), f"launch {k}"
    assert np.array_equal(last.cpu().numpy(), with_s)
    assert dataclasses.replace(_cfg(1, 1, 1), split_spheres=True).flags() & rt.RTC_F_SPLIT_SPHERES
