"""The sky pass's sample loop with its path decided once per strip (rtc_sky.h sky_samples_on, rtc_device.h env_classify /
environment_miss_body) against the CPU oracle, bit for bit: the u8 frame, the float accumulator and the segment
counter wherever the route returns them.

Frames: 96x54 with one small triangle in a corner (the second strip of every row is cut by the frame's edge) and 160x24
with the cube model in front of the camera (its pixels are the geometry kernel's, so the strips around it hold both kinds).
spp 1, 2, 3 and 64: the unrolled loop's remainder.  Cameras at the origin: looking up (every strip on powf_sky_unit's
path), down (no strip evaluates the sky powf), level (the horizon inside the frame: whole rows on either side) and level
and rolled by 20 degrees (strips that cross the horizon: powf_glibc_pos).  Environments: the headline's; a sun that never
vanishes (a zero colour component: env_vanish_limit gives -inf); intensity 0 and negative; focus 0, negative, an odd
integer, +inf and NaN (pow_ref's cases).  Routes: the pipelined launch without an accumulator (the instantiation without
the GENERAL code), the joined launch with the accumulator, hoisted primaries, a pipelined 1/4 row share (the merged sky
pass) and two passes of rtc_render_samples_async.

The CPU tests restate env_classify in numpy on the same frames: every path the loop is specialised for occurs in them, and
on every strip classified "sun term known" the oracle's pixel sums with and without the sun are the same bits."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
from conftest import load_tris

from env_edge_scenes import (EDGE_SUN, GROUND, HORIZON, ZENITH, _default_record, camera_towards, corner_triangle, pixel_sum,
                             primary_rays, scene_record, scene_struct)

import oracle.binding as orc
import raytracingc_amd as rt
from raytracingc_amd._abi import RtcCamera, RtcRenderDesc, Vec3

MAX_BOUNCE = 10
FRAMES = {"96x54": (96, 54), "160x24": (160, 24)}
SPPS = (1, 2, 3, 64)
SPLITS = {1: [1], 2: [1, 1], 3: [1, 2], 64: [3, 61]}  # the passes of the two-pass route (one sample: one pass)
CAMERAS = ("up", "down", "level", "rolled")
INF, NAN = math.inf, math.nan
# name -> scene record (focus, intensity); the sun of env_edge_scenes' edge frames, low in the sky
ENVS = {
    "headline": _default_record(),
    "never_vanish": scene_record(EDGE_SUN, HORIZON, (0.3, 0.9, 0.0), GROUND, 22.0, 0.75),
    "i_zero": scene_record(EDGE_SUN, HORIZON, ZENITH, GROUND, 22.0, 0.0),
    "i_neg": scene_record(EDGE_SUN, HORIZON, ZENITH, GROUND, 22.0, -0.75),
    "f_zero": scene_record(EDGE_SUN, HORIZON, ZENITH, GROUND, 0.0, 0.75),
    "f_neg": scene_record(EDGE_SUN, HORIZON, ZENITH, GROUND, -1.5, 0.75),
    "f_odd": scene_record(EDGE_SUN, HORIZON, ZENITH, GROUND, 3.0, 0.75),
    "f_inf": scene_record(EDGE_SUN, HORIZON, ZENITH, GROUND, INF, 0.75),
    "f_nan": scene_record(EDGE_SUN, HORIZON, ZENITH, GROUND, NAN, 0.75),
}
ROUTES = ("pipelined_fast", "joined_accum", "hoisted", "merged_share", "two_passes")
SHARE = dict(row_start=1, row_stride=4)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _v(a):
    return np.array([a.x, a.y, a.z], np.float64)


def _camera(frame, which):
    """A camera at the origin; fov 2.4 W / H keeps every pixel within 27 degrees of the viewing direction."""
    W, H = FRAMES[frame]
    fov = 2.4 * W / H
    towards = {"up": (0.3, -1.0, 0.2), "down": (0.3, 1.0, 0.2), "level": (1.0, 0.0, 0.3), "rolled": (1.0, 0.0, 0.3)}[which]
    cam = camera_towards(towards, fov)
    if which != "rolled":
        return cam
    a = math.radians(20.0)
    ex, ey = _v(cam.ex), _v(cam.ey)
    return RtcCamera(cam.origin, Vec3(*(math.cos(a) * ex + math.sin(a) * ey)), Vec3(*(math.cos(a) * ey - math.sin(a) * ex)),
                     cam.ez, cam.fov)


@functools.lru_cache(maxsize=None)
def _geometry(frame, which):
    """(camera, triangles): the corner triangle, or the cube model scaled and moved in front of the camera, about 72 pixels
    wide around the frame's centre (the strips [0, 64) and [64, 128) of its rows hold cube and sky pixels)."""
    W, H = FRAMES[frame]
    cam = _camera(frame, which)
    if frame == "96x54":
        return cam, corner_triangle(cam, W, H)
    tris = load_tris("cube")[0].copy()
    pts = np.stack([[tris[k][c] for c in "xyz"] for k in ("posA", "posB", "posC")]).astype(np.float64)  # [3, 3, n]
    lo, hi = pts.min((0, 2)), pts.max((0, 2))
    centre, half = (lo + hi) / 2, float((hi - lo).max()) / 2
    dist = 10.0
    scale = (3.0 * dist / cam.fov) / half
    ez = _v(cam.ez)
    for k in ("posA", "posB", "posC"):
        for i, c in enumerate("xyz"):
            tris[k][c] = ((tris[k][c].astype(np.float64) - centre[i]) * scale + dist * ez[i]).astype(np.float32)
    return cam, tris


@functools.lru_cache(maxsize=None)
def _oracle(frame, which, env, spp, share):
    """The oracle's (u8 rows, accumulator rows, segments): once per case, shared, read-only."""
    W, H = FRAMES[frame]
    cam, tris = _geometry(frame, which)
    d = RtcRenderDesc(W, H, spp, MAX_BOUNCE, 1, 1 if share else 0, 4 if share else 1, 0, 0)
    col, acc, seg = orc.render(tris, None, scene_struct(ENVS[env]), cam, d, threads=8)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


# ---- env_classify restated (CPU) -------------------------------------------------------------------------------------
SKY_UNIT, SKY_POS, SKY_NONE = 0, 1, 2
SUN_NONE, SUN_POW, SUN_POW_ODD, SUN_SPECIAL = 0, 1, 2, 3


def _smoothstep(inf, sup, x):
    """moremath.c:49-53 in float32 (rtc_device.h smoothstep_k is bit-identical to it for every x)."""
    f = np.float32
    with np.errstate(all="ignore"):
        t = ((x.astype(f) - f(inf)) / (f(sup) - f(inf))).astype(f)
        t = np.where(t < 0, f(0), np.where(t > 1, f(1), t)).astype(f)
        return ((t * t).astype(f).astype(np.float64) * (3.0 - 2.0 * t.astype(np.float64))).astype(f)


def _checkint(iy):
    """e_powf.c checkint: 0 not an integer, 1 odd, 2 even."""
    e = (iy >> 23) & 0xff
    if e < 0x7f:
        return 0
    if e > 0x7f + 23:
        return 2
    if iy & ((1 << (0x7f + 23 - e)) - 1):
        return 0
    return 1 if iy & (1 << (0x7f + 23 - e)) else 2


def classify(rec, d, live):
    """env_classify for the strips of one frame: d float32 [rows, W, 3] primary directions, live [rows, W] the sky pixels.
    Returns {(row, first column): (sky path, sun path)} for the 64-pixel strips with a live lane.  The tests are the kernel's
    (rtc_device.h env_classify, sun_vanishes with numpy's log2 for powf_log2: equal away from the limit's last bits)."""
    f = np.float32
    sun = np.array([rec["normalizedSunDirection"][c] for c in "xyz"], f)
    focus, intensity = f(rec["sunFocus"]), f(rec["sunIntensity"])
    with np.errstate(all="ignore"):
        sa = _smoothstep(0.0, 0.74, -d[..., 1]).view(np.uint32)
        dot = ((d[..., 0] * sun[0]).astype(f) + (d[..., 1] * sun[1]).astype(f)).astype(f)
        dot = (dot + (d[..., 2] * sun[2]).astype(f)).astype(f)
        x = np.where((dot < 0) | np.isnan(dot), f(0), dot).astype(f)  # fmax0_ref
        ix = x.view(np.uint32)
        mask = d[..., 1] < 0
        skip = bool(focus > 0) and bool(intensity - intensity == 0)  # env_sun_skippable
        lim = rt.env_vanish_limit(rec)
        ok = mask & (ix >= 0x00800000) & (ix < 0x3f800000) & (lim > -1e300)
        vanish = np.zeros(x.shape, bool)
        vanish[ok] = float(focus) * np.log2(x[ok].astype(np.float64)) < lim
        known = (skip & (ix != 0x80000000) & ((x == 0) | (~mask & (x <= 1)))) | vanish
    unit = (sa - np.uint32(0x00800000)) <= np.uint32(0x3f800000 - 0x00800000)
    iy = int(np.array(focus).view(np.uint32))
    special = (2 * iy - 1) % (1 << 32) >= 2 * 0x7f800000 - 1  # powf_zeroinfnan
    computed = SUN_SPECIAL if special else (SUN_POW_ODD if _checkint(iy) == 1 else SUN_POW)
    out = {}
    rows, W = live.shape
    for r in range(rows):
        for c in range(0, W, 64):
            m = live[r, c:c + 64]
            if not m.any():
                continue
            sky = SKY_UNIT if unit[r, c:c + 64][m].all() else (SKY_POS if (sa[r, c:c + 64][m] != 0).any() else SKY_NONE)
            out[r, c] = (sky, SUN_NONE if known[r, c:c + 64][m].all() else computed)
    return out


@functools.lru_cache(maxsize=None)
def _classified(frame, which, env):
    W, H = FRAMES[frame]
    cam, tris = _geometry(frame, which)
    rays = primary_rays(cam, W, H)
    hit = np.zeros(len(rays), bool)
    for t in tris:  # (a pixel with a primary hit is not a sky pixel, whichever triangle)
        hit |= orc.ray_triangle(rays, np.repeat(t[None], len(rays)))[0] != 0
    d = np.stack([rays["dir"][c] for c in "xyz"], 1).astype(np.float32).reshape(H, W, 3)
    return rays, ~hit, classify(ENVS[env], d, (~hit).reshape(H, W))


def test_every_path_occurs():
    """The frames hold strips on every path of the specialised loop: the three sky paths each with the sun term known and
    computed, and pow_ref's three cases of a computed sun term; the up camera's strips are all on the unit path, the down
    camera's all without a sky powf, and only the rolled camera has strips crossing the horizon."""
    seen = set()
    for frame in FRAMES:
        for which in CAMERAS:
            for env in ENVS:
                paths = set(_classified(frame, which, env)[2].values())
                seen |= paths
                skies = {p[0] for p in paths}
                if which == "up":
                    assert skies == {SKY_UNIT}
                if which == "down":
                    assert skies == {SKY_NONE}
                if which == "level":
                    assert skies == {SKY_UNIT, SKY_NONE}
                if which == "rolled" and frame == "96x54":  # (in 160x24 the cube hides where the horizon crosses the rows)
                    assert SKY_POS in skies
    print(sorted(seen))
    for sky in (SKY_UNIT, SKY_POS, SKY_NONE):
        assert (sky, SUN_NONE) in seen and (sky, SUN_POW) in seen
    assert {p[1] for p in seen} == {SUN_NONE, SUN_POW, SUN_POW_ODD, SUN_SPECIAL}


@pytest.mark.parametrize("env", sorted(ENVS))
def test_known_sun_term_adds_nothing(env):
    """On every sky pixel of a strip classified SUN_NONE the pixel's sum (main.c:97-99 on the oracle's
    getEnvironmentLight, 1 and 3 samples) is the same bits with the sun as with an intensity of the same-signed zero: the
    decision made once per strip is right for each of its lanes, as the per-sample test's was."""
    rec = ENVS[env]
    nosun = rec.copy()
    nosun["sunIntensity"] = math.copysign(0.0, float(rec["sunIntensity"])) if not math.isnan(rec["sunIntensity"]) else 0.0
    checked = 0
    for frame in FRAMES:
        W, H = FRAMES[frame]
        for which in CAMERAS:
            rays, sky, paths = _classified(frame, which, env)
            sel = np.zeros((H, W), bool)
            for (r, c), p in paths.items():
                if p[1] == SUN_NONE:
                    sel[r, c:c + 64] = True
            sel = sel.reshape(-1) & sky
            if not sel.any():
                continue
            a = orc.environment(rays[sel], np.repeat(rec[None], int(sel.sum())))
            b = orc.environment(rays[sel], np.repeat(nosun[None], int(sel.sum())))
            for spp in (1, 3):
                assert np.array_equal(_bits(pixel_sum(a, spp)), _bits(pixel_sum(b, spp))), f"{env} {frame} {which} spp {spp}"
            checked += int(sel.sum())
    print(f"{env}: {checked} pixels in strips whose sun term is known")
    if env in ("headline", "i_zero", "i_neg", "f_odd", "never_vanish"):  # (focus > 0, finite intensity: some strip skips)
        assert checked > 0


# ---- the frames on the GPU -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_scene(frame, which):
    return rt.DeviceScene(_geometry(frame, which)[1], None)


def _render(frame, which, env, spp, route):
    """(u8, accumulator or None, segments or None) of the route."""
    import torch

    W, H = FRAMES[frame]
    cam, tris = _geometry(frame, which)
    scene = scene_struct(ENVS[env])
    if route in ("joined_accum", "hoisted"):
        col, acc, st = rt.render(tris, None, scene, cam, rt.RenderConfig(W, H, spp, MAX_BOUNCE, True, hoist=route == "hoisted"),
                                 want_accum=True)
        return col, acc, st["segments"]
    ds = _device_scene(frame, which)
    if route == "two_passes":
        cfg = rt.RenderConfig(W, H, spp, MAX_BOUNCE, True)
        col = torch.full((H, W, 3), 0xFF, dtype=torch.uint8, device="cuda")
        acc = torch.full((H, W, 3), -1, dtype=torch.int32, device="cuda")
        rng = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda")
        st, done = torch.cuda.current_stream().cuda_stream, 0
        for count in SPLITS[spp]:
            ds.render_samples_async(scene, cam, cfg, done, count, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), seg.data_ptr(),
                                    st)
            done += count
        torch.cuda.synchronize()
        return col.cpu().numpy(), acc.cpu().numpy().view(np.float32), int(seg.cpu().numpy()[0])
    share = route == "merged_share"
    cfg = rt.RenderConfig(W, H, spp, MAX_BOUNCE, True, overlap=True, **(SHARE if share else {}))
    rows = cfg.rows()
    col = torch.zeros((rows, W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((rows, W, 3), dtype=torch.float32, device="cuda") if share else None
    torch.cuda.synchronize()
    st, ev = torch.cuda.Stream(), torch.cuda.Event()
    ds.set_frame_event(ev.cuda_event)
    ds.render_rows_async(scene, cam, cfg, col.data_ptr(), accum_ptr=acc.data_ptr() if share else None, stream=st.cuda_stream)
    ev.synchronize()
    torch.cuda.synchronize()
    return col.cpu().numpy(), acc.cpu().numpy() if share else None, None


@pytest.mark.gpu
@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("which", CAMERAS)
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_sky_paths_match_oracle(frame, which, env, gpu_available):
    """Every spp on every route: the u8 frame; the accumulator's NaN positions and the bits of every other value; the segment
    count (joined, hoisted and the passes; a pipelined launch has no counters)."""
    for spp in SPPS:
        for route in ROUTES:
            ocol, oacc, oseg = _oracle(frame, which, env, spp, route == "merged_share")
            gcol, gacc, gseg = _render(frame, which, env, spp, route)
            what = f"{frame} {which} {env} spp {spp} {route}"
            assert np.array_equal(gcol, ocol), f"{what}: {int((gcol != ocol).any(-1).sum())} u8 pixels differ"
            if gacc is not None:
                nan = np.isnan(oacc)
                assert np.array_equal(np.isnan(gacc), nan), what
                bad = int(((_bits(gacc) != _bits(oacc)) & ~nan).any(-1).sum())
                assert bad == 0, f"{what}: {bad} pixels' accumulator bits differ"
            assert gseg is None or gseg == oseg, f"{what}: segments {gseg} vs {oseg}"
