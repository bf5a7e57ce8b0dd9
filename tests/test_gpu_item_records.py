"""The split launch's item records: rtc_tile_cull appends, per geometry pixel, a 16-byte record -- x | launch
row << 16 and the bits of the pixel's primary direction, which its lane holds -- and rtc_render_chain takes the pixel and its
ray from it instead of rebuilding the ray from the camera for 64 lanes.

1. The records themselves (rtc_probe_item_records: a launch's preparation and culls, no render kernel): their (x, row) are
   exactly the set bits of pixMask, each once, and their three floats are bit-equal to a float32 numpy restatement of
   main.c:88-93 with moremath.c:7-17's operation order.
2. Frames through every instantiation that reads the records, against the CPU oracle bit for bit.
3. Pipelined frames over alternating cameras: a frame never reads a neighbouring slot's records."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from conftest import load_tris
from primary_rays import launch_rows as _launch_rows, primary_dirs as _primary_dirs
from sphere_scenes import open5

import oracle.binding as orc
import raytracingc_amd as rt
from raytracingc_amd._abi import RtcRenderDesc

pytestmark = pytest.mark.gpu

# a non-default origin and fov
CAM_ARGS = ((-4.0, -1.9, -5.2), (0.6, -1.0, 1.3), 1.1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_records(tris, spheres, cam, cfg, expect_wide=False, min_x=0):
    scene = rt.default_scene()
    p = rt.item_records_probe(tris, spheres, scene, cam, cfg)
    rec, tx = p["records"], p["tiles_x"]
    rows = cfg.rows()
    assert p["wide"] == expect_wide
    assert tx == 2 * ((cfg.width + 15) // 16) and p["tiles"] == tx * 2 * ((rows + 15) // 16)
    assert (p["counts"] <= p["cap"]).all() and len(rec) == int(p["counts"].sum())
    d0 = rec[:, 0].astype(np.int64)
    if p["wide"]:
        tile, bit = d0 >> 6, d0 & 63
        x, r = (tile % tx) * 8 + (bit & 7), (tile // tx) * 8 + (bit >> 3)
    else:
        x, r = d0 & 0xFFFF, d0 >> 16
        tile, bit = (r >> 3) * tx + (x >> 3), ((r & 7) << 3) | (x & 7)
    # the set bits of pixMask, each once (and only pixels of the launch)
    assert len(rec) > 0 and (x < cfg.width).all() and (r < rows).all()
    assert int(x.max()) >= min_x
    got = np.sort(tile * 64 + bit)
    assert (np.diff(got) > 0).all(), "a pixel has two records"
    pm = p["pix_mask"]
    tbits = (pm[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    want = np.flatnonzero(tbits.reshape(-1))
    assert np.array_equal(got, want), "the records are not the set bits of pixMask"
    # sub-list l holds the tiles t = l mod 16, in the order of `counts`
    lists = np.repeat(np.arange(16), p["counts"])
    assert np.array_equal(tile % 16, lists)
    # the ray
    y = _launch_rows(cfg)[r]
    want_dir = _primary_dirs(cam, cfg, x, y)
    bad = (_bits(want_dir) != rec[:, 1:4]).any(-1)
    assert not bad.any(), f"{int(bad.sum())} of {len(rec)} records' direction bits differ from main.c:88-93"


RECORD_SHAPES = {
    "one_tile": dict(width=8, height=8),
    "edge_9x7": dict(width=9, height=7),
    "edge_101x53": dict(width=101, height=53),
    "interleaved": dict(width=96, height=54, row_start=3, row_stride=8),
    "banded": dict(width=96, height=54, row_start=8, row_stride=2, row_band=8),
}


@pytest.mark.parametrize("shape", sorted(RECORD_SHAPES))
def test_records_are_the_pixel_mask_and_the_ray(shape, gpu_available):
    tris, _ = load_tris("ultracomplex")
    cfg = rt.RenderConfig(spp=1, max_bounce=10, triangles_only=True, **RECORD_SHAPES[shape])
    _check_records(tris, None, rt.camera_basis(*CAM_ARGS), cfg)
    _check_records(tris, None, rt.camera_basis(), cfg)


def _camera_with_model_at(dx):
    """The default camera turned about the vertical axis so that the model's centre lies at main.c:88's dx (a very wide,
    8-row frame sees it 4 dx columns right of its middle column)."""
    o, c = np.array(rt.DEFAULT_ORIGIN, np.float64), np.array(rt.DEFAULT_LOOKING_AT, np.float64)
    to = c - o
    th = np.arctan(float(dx))
    for sign in (1.0, -1.0):
        cs, sn = np.cos(sign * th), np.sin(sign * th)
        look = o + np.array([cs * to[0] + sn * to[2], to[1], -sn * to[0] + cs * to[2]])
        cam = rt.camera_basis(tuple(o), tuple(look), 1.0)
        ex, ez = np.array([cam.ex.x, cam.ex.y, cam.ex.z]), np.array([cam.ez.x, cam.ez.y, cam.ez.z])
        if to @ ex > 0 and to @ ez > 0:
            return cam
    raise AssertionError("no such camera")


def test_records_pack_16_bit_columns(gpu_available):
    """4,000 x 8 with the model around column 2,800: x above 2,047 in the 16-bit field."""
    tris, _ = load_tris("ultracomplex")
    cfg = rt.RenderConfig(4000, 8, 1, 10, True)
    _check_records(tris, None, _camera_with_model_at((2800 - 2000) / 4), cfg, min_x=2048)


def test_records_of_a_launch_wider_than_16_bits(gpu_available):
    """70,000 x 8 with the model around column 67,000: more than 65,535 columns, so the records keep tile * 64 + bit
     -- and the ray all the same."""
    tris, _ = load_tris("ultracomplex")
    cfg = rt.RenderConfig(70000, 8, 1, 10, True)
    _check_records(tris, None, _camera_with_model_at((67000 - 35000) / 4), cfg, expect_wide=True, min_x=65536)


def test_records_sphere_split(gpu_available):
    """rtc_tile_cull_sph: sphere pixels are geometry pixels and get the same records."""
    tris, _ = load_tris("ultracomplex")
    cfg = rt.RenderConfig(101, 53, 1, 10, False, split_spheres=True)
    _check_records(tris, open5(), rt.camera_basis(*CAM_ARGS), cfg)


# ---- frames ------------------------------------------------------------------------------------------------------
FRAMES = {"ultra_96x54x8": ("ultracomplex", None, 96, 54, 8), "ultra_101x53x5": ("ultracomplex", None, 101, 53, 5),
          "open5_96x54x8": ("ultracomplex", "open5", 96, 54, 8)}
# the routes that read the records: joined whole frames give items deferred sample slots (GENERAL), chain_inline sums
# in-kernel, overlap is the pipelined launch, hoist the hoisted instantiation; a pipelined small share runs the merged
# sky pass
ROUTES = {
    "joined_deferred": dict(),
    "joined_inline": dict(chain_inline=True),
    "pipelined": dict(overlap=True),
    "hoisted": dict(hoist=True),
    "pipelined_hoisted": dict(overlap=True, hoist=True),
    "share_merged_sky": dict(overlap=True, row_start=1, row_stride=4),
    "share_banded": dict(overlap=True, row_start=8, row_stride=2, row_band=8),
}


@functools.lru_cache(maxsize=None)
def _frame_scene(frame):
    name, sph, W, H, spp = FRAMES[frame]
    return load_tris(name)[0], (open5() if sph else None), rt.default_scene(), rt.camera_basis(*CAM_ARGS)


@functools.lru_cache(maxsize=None)
def _device_scene(frame):
    tris, sph, _, _ = _frame_scene(frame)
    return rt.DeviceScene(tris, sph)


@functools.lru_cache(maxsize=None)
def _oracle(frame, row_start, row_stride, row_band):
    """The oracle's (u8, floats, segments) of the frame's rows, computed once per share and left unchanged."""
    tris, sph, scene, cam = _frame_scene(frame)
    _, _, W, H, spp = FRAMES[frame]
    col, acc, seg = orc.render(tris, sph, scene, cam,
                               RtcRenderDesc(W, H, spp, 10, int(sph is None), row_start, row_stride, 0, row_band), threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_frames_equal_the_oracle(frame, route, gpu_available):
    import torch

    _, sph, W, H, spp = FRAMES[frame]
    _, _, scene, cam = _frame_scene(frame)
    cfg = rt.RenderConfig(W, H, spp, 10, sph is None, split_spheres=sph is not None, **ROUTES[route])
    ocol, oacc, oseg = _oracle(frame, cfg.row_start, cfg.row_stride, cfg.row_band)
    ds = _device_scene(frame)
    rows = cfg.rows()
    st = torch.cuda.current_stream().cuda_stream
    # the route itself (a launch that counts segments is always a joined one), then the same launch counting
    for counters in (False, True):
        out = torch.zeros((rows, W, 3), dtype=torch.uint8, device="cuda")
        acc = torch.zeros((rows, W, 3), dtype=torch.float32, device="cuda")
        seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
        torch.cuda.synchronize()
        ds.render_rows_async(scene, cam, cfg, out.data_ptr(), acc.data_ptr(), seg.data_ptr() if counters else None, st)
        torch.cuda.synchronize()
        col, a = out.cpu().numpy(), acc.cpu().numpy()
        what = f"{frame} {route} counters={counters}"
        assert np.array_equal(col, ocol), f"{what}: {int((col != ocol).any(-1).sum())} u8 pixels differ"
        bad = int((_bits(a) != _bits(oacc)).any(-1).sum())
        assert bad == 0, f"{what}: {bad} pixels' accumulator bits differ"
        if counters:
            assert int(seg.cpu().numpy()[0]) == oseg, f"{what}: segments"


def test_pipelined_frames_read_their_own_records(gpu_available):
    """Six pipelined frames over three alternating cameras (rtc_frame_loop_cameras: RTC_F_OVERLAP launches cycling through
    the scratch slots, each with its own list region): every frame equals its own single render."""
    import torch

    tris, _ = load_tris("ultracomplex")
    scene = rt.default_scene()
    cams = [rt.camera_basis(), rt.camera_basis(*CAM_ARGS), rt.camera_basis((-5.3, -1.2, -4.1), (1.2, -1.4, 0.7), 0.9)]
    W, H, spp, frames = 96, 54, 8, 6
    refs = [rt.render(tris, None, scene, c, rt.RenderConfig(W, H, spp, 10, True))[0] for c in cams]
    ds = rt.DeviceScene(tris, None)
    st = torch.cuda.Stream()
    dev = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(frames)]
    torch.cuda.synchronize()  # (the zero fills ran on the current stream, not the launch stream)
    host = [torch.zeros((H, W, 3), dtype=torch.uint8, pin_memory=True) for _ in range(frames)]
    out = ds.frame_loop(scene, cams, rt.RenderConfig(W, H, spp, 10, True), [d.data_ptr() for d in dev],
                        [h.data_ptr() for h in host], W * 3, frames, st.cuda_stream)
    assert out["frames"] == frames
    for k in range(frames):
        assert np.array_equal(host[k].numpy(), refs[k % 3]), f"frame {k}"
    ds.close()
