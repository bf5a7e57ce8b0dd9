"""Where rtc_render_chain stores an item's result (rtc_chain.h, the item tail): frames at the two ends of its
item loop against the CPU oracle, bit for bit -- the u8 frame, the float accumulator and the segment counter wherever the
route returns them.  Written with round 11's deferred store (an item's result stored by the wave's next item, or after the
loop; measured, not kept: DESIGN §7) and kept as the check any such change has to pass.

few: 32x32 with one small triangle -- far fewer geometry pixels than the kernel has waves, so a wave has no item (and must
store nothing) or one (its last).  full: 128x72 filled by one large triangle, 4 spp -- 9,216 items, so every workgroup of a
whole-frame launch takes at least 8 and nearly every item is followed by another of the same wave.  Routes: the
pipelined launch summing in-kernel (the instantiation without the GENERAL code), joined launches with the accumulator
(deferred sample slots, and in-kernel sums), a pipelined 1/8 row share (the merged sky pass: the per-item colour words) and
two passes of rtc_render_samples_async (the pixel's state and accumulator).  Three pipelined frames of three cameras go
into three buffers without a wait between them: a store that landed in another frame's buffer would show in both."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from env_edge_scenes import camera_towards, corner_triangle, primary_rays

import oracle.binding as orc
import raytracingc_amd as rt
from raytracingc_amd._abi import TRIANGLE_DT, RtcRenderDesc

MAX_BOUNCE, SPP = 10, 4
FRAMES = {"few": (32, 32), "full": (128, 72)}
VIEWS = [(1.0, -0.2, 0.3), (1.0, -0.15, 0.33), (0.97, -0.22, 0.27)]  # the camera of every test, and two close to it
FOV = 8.0
ROUTES = ("pipelined_fast", "joined_deferred", "joined_inline", "merged_share", "two_passes")
SHARE = dict(row_start=3, row_stride=8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _wall(cam, W, H):
    """One diffuse triangle facing the camera 10 units away, its corners at the pixels (-W, -H), (5W, -H) and (-W, 5H): it
    fills the frame, and the frames of the cameras close by (no edge crosses them)."""
    ex, ey, ez = (np.array([a.x, a.y, a.z], np.float64) for a in (cam.ex, cam.ey, cam.ez))

    def at(px, py):
        return tuple(10.0 * (ex * ((px - W // 2) / (H // 2)) + ey * ((py - H // 2) / (H // 2)) + ez * cam.fov) / cam.fov)

    t = np.zeros(1, TRIANGLE_DT)
    t[0]["posA"], t[0]["posB"], t[0]["posC"] = at(-W, -H), at(5 * W, -H), at(-W, 5 * H)
    t[0]["normal"] = tuple(-ez)
    t[0]["mat"]["color"] = (0.8, 0.7, 0.6)
    t[0]["mat"]["emissionStrength"] = 0.0
    t[0]["mat"]["smoothness"] = 0.25
    return t


@functools.lru_cache(maxsize=None)
def _geometry(frame):
    """(triangles, the three cameras)."""
    W, H = FRAMES[frame]
    cams = [camera_towards(v, FOV) for v in VIEWS]
    return (corner_triangle(cams[0], W, H) if frame == "few" else _wall(cams[0], W, H)), cams


@functools.lru_cache(maxsize=None)
def _oracle(frame, view, share):
    """The oracle's (u8 rows, accumulator rows, segments): once per case, shared, read-only."""
    W, H = FRAMES[frame]
    tris, cams = _geometry(frame)
    d = RtcRenderDesc(W, H, SPP, MAX_BOUNCE, 1, SHARE["row_start"] if share else 0, SHARE["row_stride"] if share else 1, 0, 0)
    col, acc, seg = orc.render(tris, None, rt.default_scene(), cams[view], d, threads=8)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


def test_frames_hold_what_they_are_meant_to():
    """few: between 8 and 64 pixels with a primary hit (a launch has thousands of waves).  full: every pixel of each of the
    three cameras' frames has one, and the three frames differ."""
    W, H = FRAMES["few"]
    tris, cams = _geometry("few")
    hits = int((orc.ray_triangle(primary_rays(cams[0], W, H), np.repeat(tris, W * H))[0] != 0).sum())
    print(f"few: {hits} pixels with a primary hit")
    assert 8 <= hits <= 64
    W, H = FRAMES["full"]
    tris, cams = _geometry("full")
    for v, cam in enumerate(cams):
        rays = primary_rays(cam, W, H)
        hit = np.zeros(W * H, bool)
        for t in tris:
            hit |= orc.ray_triangle(rays, np.repeat(t[None], W * H))[0] != 0
        assert hit.all(), f"view {v}: {int((~hit).sum())} pixels see the sky"
    cols = [_oracle("full", v, False)[0] for v in range(3)]
    assert (cols[0] != cols[1]).any() and (cols[1] != cols[2]).any() and (cols[0] != cols[2]).any()


@functools.lru_cache(maxsize=None)
def _device_scene(frame):
    return rt.DeviceScene(_geometry(frame)[0], None)


def _pipelined(ds, cam, cfg, want_accum):
    """One pipelined launch on a stream of its own, complete at its frame event."""
    import torch

    col = torch.zeros((cfg.rows(), cfg.width, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((cfg.rows(), cfg.width, 3), dtype=torch.float32, device="cuda") if want_accum else None
    torch.cuda.synchronize()
    st, ev = torch.cuda.Stream(), torch.cuda.Event()
    ev.record(st)
    ds.set_frame_event(ev.cuda_event)
    ds.render_rows_async(rt.default_scene(), cam, cfg, col.data_ptr(), accum_ptr=acc.data_ptr() if want_accum else None,
                         stream=st.cuda_stream)
    ev.synchronize()
    torch.cuda.synchronize()
    return col.cpu().numpy(), acc.cpu().numpy() if want_accum else None, None


def _render(frame, route):
    """(u8, accumulator or None, segments or None) of the route."""
    import torch

    W, H = FRAMES[frame]
    tris, cams = _geometry(frame)
    cam, scene = cams[0], rt.default_scene()
    if route in ("joined_deferred", "joined_inline"):
        cfg = rt.RenderConfig(W, H, SPP, MAX_BOUNCE, True, chain_inline=route == "joined_inline")
        col, acc, st = rt.render(tris, None, scene, cam, cfg, want_accum=True)
        return col, acc, st["segments"]
    ds = _device_scene(frame)
    if route == "pipelined_fast":
        return _pipelined(ds, cam, rt.RenderConfig(W, H, SPP, MAX_BOUNCE, True, overlap=True, chain_inline=True), False)
    if route == "merged_share":
        return _pipelined(ds, cam, rt.RenderConfig(W, H, SPP, MAX_BOUNCE, True, overlap=True, **SHARE), True)
    cfg = rt.RenderConfig(W, H, SPP, MAX_BOUNCE, True, chain_inline=True)
    col = torch.full((H, W, 3), 0xFF, dtype=torch.uint8, device="cuda")
    acc = torch.full((H, W, 3), -1, dtype=torch.int32, device="cuda")
    rng = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda")
    st, done = torch.cuda.current_stream().cuda_stream, 0
    for count in (1, SPP - 1):
        ds.render_samples_async(scene, cam, cfg, done, count, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), seg.data_ptr(), st)
        done += count
    torch.cuda.synchronize()
    return col.cpu().numpy(), acc.cpu().numpy().view(np.float32), int(seg.cpu().numpy()[0])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_frame_matches_oracle(frame, route, gpu_available):
    ocol, oacc, oseg = _oracle(frame, 0, route == "merged_share")
    gcol, gacc, gseg = _render(frame, route)
    what = f"{frame} {route}"
    assert np.array_equal(gcol, ocol), f"{what}: {int((gcol != ocol).any(-1).sum())} u8 pixels differ"
    if gacc is not None:
        bad = int((_bits(gacc) != _bits(oacc)).any(-1).sum())
        assert bad == 0, f"{what}: {bad} pixels' accumulator bits differ"
    assert gseg is None or gseg == oseg, f"{what}: segments {gseg} vs {oseg}"


@pytest.mark.gpu
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_three_pipelined_frames_keep_their_buffers(frame, gpu_available):
    """Three cameras' frames enqueued back to back on one stream, each into its own zeroed buffer: every buffer holds the
    oracle's frame of its own camera."""
    import torch

    W, H = FRAMES[frame]
    _, cams = _geometry(frame)
    ds = _device_scene(frame)
    cfg = rt.RenderConfig(W, H, SPP, MAX_BOUNCE, True, overlap=True, chain_inline=True)
    bufs = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in cams]
    torch.cuda.synchronize()
    st, evs = torch.cuda.Stream(), []
    for cam, buf in zip(cams, bufs):
        ev = torch.cuda.Event()
        ev.record(st)
        ds.set_frame_event(ev.cuda_event)
        ds.render_rows_async(rt.default_scene(), cam, cfg, buf.data_ptr(), stream=st.cuda_stream)
        evs.append(ev)
    for ev in evs:
        ev.synchronize()
    torch.cuda.synchronize()
    for v, buf in enumerate(bufs):
        ocol = _oracle(frame, v, False)[0]
        got = buf.cpu().numpy()
        assert np.array_equal(got, ocol), f"{frame} view {v}: {int((got != ocol).any(-1).sum())} u8 pixels differ"
