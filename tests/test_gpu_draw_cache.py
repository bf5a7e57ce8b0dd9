"""The draw cache (rtc.h rtc_scene_set_draw_cache): per pixel that has seen geometry, the 64 hit draws of its
seed, filled once behind the tile cull and read by rtc_render_chain's first window in every later launch.  The cache never
changes a frame, so every frame here is compared bit for bit -- u8 and accumulator -- with the same launch under
RTC_F_NO_DRAW_CACHE and with the CPU oracle (as tests/test_gpu_chain_paths.py does), and the cache's own report
(DeviceScene.draw_cache_stats, draw_cache_block) with what the launch must have done: which items were fresh, which had no
block, what a block holds.  Small frames (64 x 48 and below); the launches are those that run the geometry kernel without
its GENERAL code (in-kernel sums: chain_inline, or pipelined row shares), which chain_report confirms.  No reference
counterpart: the values cached are moremath.c:89-108's, drawn from main.c:95's seed."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

import oracle.binding as orc
import raytracingc_amd as rt
from chain_path_scenes import FRAMES as BOX_FRAMES, SCENES as BOX_SCENES
from conftest import load_tris
from raytracingc_amd.distributed import band_rows

pytestmark = pytest.mark.gpu

W, H = 64, 48
CUBE_CAMERA = ((-4.0, -3.08, 0.0), (0.0, -1.58, 0.0), 3.5)  # (tests/test_gpu_scene_update.py: the cube fills a good part)
CUBE_MOVED = ((-3.7, -3.0, 0.4), (0.0, -1.58, 0.0), 3.5)
SCENES = {"cube": (CUBE_CAMERA, CUBE_MOVED), "simplest": ((), ((-4.5, -1.5, -4.75),))}
INLINE = dict(chain_inline=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _tris(name):
    return BOX_SCENES[name][0] if name in BOX_SCENES else load_tris(name)[0]


@functools.lru_cache(maxsize=None)
def _oracle(name, cam_args, w, h, spp, mb, row_start=0, row_stride=1, row_band=0):
    """The oracle's (u8, floats) of the launch's rows, computed once and left unchanged; cam_args: camera_basis', or a
    chain-path scene's own camera (None)."""
    cam = BOX_SCENES[name][1] if cam_args is None else rt.camera_basis(*cam_args)
    d = rt.RenderConfig(w, h, spp, mb, True, row_start=row_start, row_stride=row_stride, row_band=row_band).desc()
    col, acc, _ = orc.render(_tris(name), None, rt.default_scene(), cam, d, threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc


def _launch(ds, cam, cfg):
    import torch

    rows = cfg.rows()
    out = torch.zeros((rows, cfg.width, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((rows, cfg.width, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_rows_async(rt.default_scene(), cam, cfg, out.data_ptr(), acc.data_ptr(), None,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()  # (the whole device: an overlapped launch ends on the scene's streams)
    rep = ds.chain_report()
    assert not rep["general"], f"the launch ran a GENERAL kernel, which never uses the cache: {rep}"
    return out.cpu().numpy(), acc.cpu().numpy()


def _equal(what, got, want):
    col, acc = got
    wcol, wacc = want
    nan = np.isnan(wacc)
    assert np.array_equal(np.isnan(acc), nan), f"{what}: NaN positions differ"
    bad = int(((_bits(acc) != _bits(wacc)) & ~nan).any(-1).sum())
    assert bad == 0, f"{what}: {bad} pixels' accumulator bits differ"
    assert np.array_equal(col, wcol), f"{what}: {int((col != wcol).any(-1).sum())} u8 pixels differ"


def _frame(what, ds, name, cam_args, cfg):
    """One launch with the cache, compared with the same launch without it and with the oracle; returns the cache's report
    after the cached launch."""
    cam = BOX_SCENES[name][1] if cam_args is None else rt.camera_basis(*cam_args)
    got = _launch(ds, cam, cfg)
    stats = ds.draw_cache_stats()
    _equal(f"{what}: against RTC_F_NO_DRAW_CACHE", got, _launch(ds, cam, dataclasses.replace(cfg, draw_cache=False)))
    assert ds.draw_cache_stats() == stats, f"{what}: the launch without the cache touched it"
    _equal(f"{what}: against the oracle", got, _oracle(name, cam_args, cfg.width, cfg.height, cfg.spp, cfg.max_bounce,
                                                       cfg.row_start, cfg.row_stride, cfg.row_band))
    return stats


def _geometry_pixels(name, cam_args, cfg):
    cam = BOX_SCENES[name][1] if cam_args is None else rt.camera_basis(*cam_args)
    return int(rt.item_records_probe(_tris(name), None, rt.default_scene(), cam, cfg)["counts"].sum())


@pytest.mark.parametrize("name", sorted(SCENES))
def test_cold_warm_and_moved_camera(name, gpu_available):
    """Frame 1 of a scene caches every geometry pixel, frame 2 none, frame 3 from a moved camera the pixels new to it."""
    cam0, cam1 = SCENES[name]
    cfg = rt.RenderConfig(W, H, 64, 10, True, **INLINE)
    geo0, geo1 = _geometry_pixels(name, cam0, cfg), _geometry_pixels(name, cam1, cfg)
    assert geo0 > 0 and geo1 > 0
    ds = rt.DeviceScene(_tris(name), None)
    try:
        assert ds.draw_cache_stats() == dict(blocks=0, capacity=0, fresh=0, uncached=0)
        cold = _frame(f"{name} cold", ds, name, cam0, cfg)
        assert cold == dict(blocks=geo0, capacity=W * H, fresh=geo0, uncached=0), cold
        warm = _frame(f"{name} warm", ds, name, cam0, cfg)
        assert warm == dict(cold, fresh=0), warm
        moved = _frame(f"{name} moved", ds, name, cam1, cfg)
        assert 0 < moved["fresh"] < geo1 and moved["uncached"] == 0, (moved, geo1)
        assert moved["blocks"] == geo0 + moved["fresh"]
        ds.draw_cache_reset()
        again = _frame(f"{name} after a reset", ds, name, cam1, cfg)
        assert again == dict(blocks=geo1, capacity=W * H, fresh=geo1, uncached=0), again
    finally:
        ds.close()


@pytest.mark.parametrize("spp", [64, 40, 7, 130])
def test_sample_counts(spp, gpu_available):
    """nAct < 64 uses the first nAct entries of a block; 130 samples take a cached first window, then computed windows at
    jn > 0.  Cold and warm."""
    ds = rt.DeviceScene(_tris("cube"), None)
    try:
        cfg = rt.RenderConfig(W, H, spp, 10, True, **INLINE)
        assert _frame(f"cube spp {spp} cold", ds, "cube", CUBE_CAMERA, cfg)["fresh"] > 0
        assert _frame(f"cube spp {spp} warm", ds, "cube", CUBE_CAMERA, cfg)["fresh"] == 0
    finally:
        ds.close()


@pytest.mark.parametrize("frame", ["box_diffuse_T", "box_gloss_mb65"])
def test_hit_heavy_boxes(frame, gpu_available):
    """The HITS instantiation: later hits read cached entries lane + iter from the draw table and compute past nAct; with
    maxBounce 65 every lane ends past it."""
    name, w, h, spp, mb = BOX_FRAMES[frame]
    ds = rt.DeviceScene(_tris(name), None)
    try:
        cfg = rt.RenderConfig(w, h, spp, mb, True, **INLINE)
        cold = _frame(f"{frame} cold", ds, name, None, cfg)
        assert ds.chain_report()["hits"] and cold["fresh"] > 0
        assert _frame(f"{frame} warm", ds, name, None, cfg) == dict(cold, fresh=0)
    finally:
        ds.close()


def _lcg(s, n):
    for _ in range(n):
        s = (s * 747796405 + 2891336453) & 0xFFFFFFFF
    return s


def test_entry_values(gpu_available):
    """Entry j of a pixel's block is RandomDiretion from the seed advanced 7 j draws and the roulette value that follows:
    bit for bit what the random_direction probe and the oracle's RNG give from that state.  The box is closed around the
    camera, so the first and the last pixel of the frame have blocks."""
    name, w, h, spp, mb = BOX_FRAMES["box_diffuse_T"]
    ds = rt.DeviceScene(_tris(name), None)
    try:
        _launch(ds, BOX_SCENES[name][1], rt.RenderConfig(w, h, spp, mb, True, **INLINE))
        for seed in (0, 1, w - 1, w, 7 * w + 5, w * h - 2, w * h - 1):
            block = ds.draw_cache_block(seed)
            assert block is not None, f"seed {seed} has no block"
            states = np.array([_lcg(seed, 7 * j) for j in range(64)], np.uint32)
            for what, src in (("the probe", rt), ("the oracle", orc)):
                u, _, d = src.random_sequences(states, 7)
                want = np.concatenate([d[:, 0, :], u[:, 6:7]], axis=1)
                bad = np.flatnonzero((_bits(block) != _bits(want)).any(-1))
                assert len(bad) == 0, f"seed {seed}: entries {bad[:8]} differ from {what}"
        assert ds.draw_cache_block(w * h) is None  # past the table
    finally:
        ds.close()


def test_pool_exhaustion(gpu_available):
    """Eight blocks: the launch mixes items with a block and items that compute their draws."""
    ds = rt.DeviceScene(_tris("cube"), None)
    try:
        ds.set_draw_cache(8)
        cfg = rt.RenderConfig(W, H, 64, 10, True, **INLINE)
        geo = _geometry_pixels("cube", CUBE_CAMERA, cfg)
        cold = _frame("cube, 8 blocks, cold", ds, "cube", CUBE_CAMERA, cfg)
        assert cold == dict(blocks=8, capacity=8, fresh=8, uncached=geo - 8), cold
        warm = _frame("cube, 8 blocks, warm", ds, "cube", CUBE_CAMERA, cfg)
        assert warm == dict(cold, fresh=0), warm
        ds.set_draw_cache(0)  # off: the launch runs the kernel without the cache
        _frame("cube, cache off", ds, "cube", CUBE_CAMERA, cfg)
        assert ds.draw_cache_stats() == dict(blocks=0, capacity=0, fresh=0, uncached=0)
    finally:
        ds.close()


def test_size_change(gpu_available):
    """Width 64, then 48, then 64 again on one scene: each change clears the cache (every geometry pixel is fresh again and
    the pool holds this frame's pixels alone), and the frames are the references'."""
    ds = rt.DeviceScene(_tris("cube"), None)
    try:
        for w in (64, 48, 64):
            cfg = rt.RenderConfig(w, H, 16, 10, True, **INLINE)
            geo = _geometry_pixels("cube", CUBE_CAMERA, cfg)
            got = _frame(f"cube at width {w}", ds, "cube", CUBE_CAMERA, cfg)
            assert got["fresh"] == geo and got["blocks"] == geo and got["uncached"] == 0, (w, got, geo)
            assert _frame(f"cube at width {w}, warm", ds, "cube", CUBE_CAMERA, cfg)["fresh"] == 0
    finally:
        ds.close()


@pytest.mark.parametrize("band", [0, 8])
def test_row_shares(band, gpu_available):
    """The two 1/2 shares of a frame (pipelined small shares: the merged sky pass) equal the whole frame's rows: a share's
    seeds are frame rows, and the second share finds the first one's table."""
    ds = rt.DeviceScene(_tris("cube"), None)
    try:
        whole = _oracle("cube", CUBE_CAMERA, W, H, 16, 10)
        fresh = []
        for rank in range(2):
            cfg = rt.RenderConfig(W, H, 16, 10, True, overlap=True, row_start=rank * (band or 1), row_stride=2, row_band=band)
            fresh.append(_frame(f"share {rank} band {band}", ds, "cube", CUBE_CAMERA, cfg)["fresh"])
            ys = band_rows(H, rank, 2, band or 1)
            got = _launch(ds, rt.camera_basis(*CUBE_CAMERA), cfg)
            _equal(f"share {rank} band {band}: the whole frame's rows", got, (whole[0][ys], whole[1][ys]))
        whole_cfg = rt.RenderConfig(W, H, 16, 10, True, **INLINE)
        assert sum(fresh) == _geometry_pixels("cube", CUBE_CAMERA, whole_cfg) and min(fresh) > 0
        assert _frame("the whole frame after its shares", ds, "cube", CUBE_CAMERA, whole_cfg)["fresh"] == 0
    finally:
        ds.close()


def test_pipelined_frames(gpu_available):
    """Eight RTC_F_OVERLAP row shares alternating two cameras, enqueued back to back on the alternating cull streams -- one
    frame's fill and the next frame's geometry kernel are in flight together -- each consumed at its frame event."""
    import torch

    ds = rt.DeviceScene(_tris("cube"), None)
    try:
        cfg = rt.RenderConfig(W, H, 16, 10, True, overlap=True, row_start=1, row_stride=2)
        cams = [CUBE_CAMERA, CUBE_MOVED]
        want = [_oracle("cube", c, W, H, 16, 10, 1, 2, 0) for c in cams]
        rows = cfg.rows()
        st = torch.cuda.Stream()
        outs = [torch.zeros((rows, W, 3), dtype=torch.uint8, device="cuda") for _ in range(8)]
        accs = [torch.zeros((rows, W, 3), dtype=torch.float32, device="cuda") for _ in range(8)]
        events = [torch.cuda.Event() for _ in range(8)]
        for ev in events:
            ev.record(st)  # (an event has no handle before its first record)
        torch.cuda.synchronize()
        for k in range(8):
            ds.set_frame_event(events[k].cuda_event)
            ds.render_rows_async(rt.default_scene(), rt.camera_basis(*cams[k % 2]), cfg, outs[k].data_ptr(),
                                 accs[k].data_ptr(), None, st.cuda_stream)
        for k in range(8):
            events[k].synchronize()
            _equal(f"pipelined frame {k}", (outs[k].cpu().numpy(), accs[k].cpu().numpy()), want[k % 2])
        torch.cuda.synchronize()
        assert not ds.chain_report()["general"]
        stats = ds.draw_cache_stats()
        assert stats["fresh"] == 0 and stats["uncached"] == 0 and stats["blocks"] > 0
    finally:
        ds.close()


def test_geometry_update(gpu_available):
    """rtc_scene_update_async between two frames: the draws do not depend on the geometry, the geometry-pixel set does."""
    import torch

    tris = _tris("cube")
    moved = tris.copy()
    for v in ("posA", "posB", "posC"):
        moved[v]["x"] = (moved[v]["x"] * np.float32(1.25) + np.float32(0.4)).astype(np.float32)
        moved[v]["z"] = (moved[v]["z"] * np.float32(1.25)).astype(np.float32)
    cam = rt.camera_basis(*CUBE_CAMERA)
    cfg = rt.RenderConfig(W, H, 16, 10, True, **INLINE)
    d = cfg.desc()
    want = orc.render(moved, None, rt.default_scene(), cam, d, threads=16)[:2]
    ds = rt.DeviceScene(tris, None)
    try:
        before = _frame("cube before the update", ds, "cube", CUBE_CAMERA, cfg)
        dev = torch.from_numpy(moved.view(np.uint8).reshape(-1)).cuda()
        ds.update(tris=dev)
        got = _launch(ds, cam, cfg)
        after = ds.draw_cache_stats()
        _equal("the updated cube: against the oracle", got, want)
        _equal("the updated cube: against RTC_F_NO_DRAW_CACHE", got, _launch(ds, cam, dataclasses.replace(cfg, draw_cache=False)))
        assert before["blocks"] == _geometry_pixels("cube", CUBE_CAMERA, cfg)
        assert after["fresh"] > 0 and after["blocks"] == before["blocks"] + after["fresh"], (before, after)
    finally:
        ds.close()
