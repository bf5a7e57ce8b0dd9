"""rtc_render_chain's in-kernel sums (rtc_chain.h flush(): a window's samples staged in LDS one row per component, then
added in sample order by lanes 0..2) against the CPU oracle, bit for bit: NaN positions equal, every other float of the
accumulator bit-equal, the u8 frame equal, the segment count equal on the counting launch.  No tolerance.

Frames of 96x54 (or a 54-row share of 96x432) get deferred sample slots by default, so every case asks for the in-kernel
sums -- RTC_F_CHAIN_INLINE joined, and RTC_F_CHAIN_INLINE | RTC_F_OVERLAP (tests/test_gpu_chain_paths.py's joined_inline and
pipelined_inline) -- and reads DeviceScene.chain_report after the launch: the kernel without the GENERAL code has no
deferred slots at all, and a GENERAL launch (segment counters, a pass) with the flag gets none from the planner.

The shapes are the smallest at which the sums can go wrong:
  spp 64             one full window: the unrolled body
  spp 1, 2, 3, 5     a last quad with 1, 2 and 3 staged entries beside unstaged dwords, windows of fewer than 64 lanes
  spp 63, 65, 130    a 63-sample window; two and three windows, the accumulator carried from flush to flush
  fsuzane, the boxes samples with several hits (single-lane staging between the runs) and primary misses inside a geometry
                     pixel's window (a flush mid-window, then more staging into the same space)
  materials          NaN, +inf, -inf and -0 samples: an unstaged dword added by mistake, or a staged one left out, shows
  16 + 48 samples    two passes: the second starts from the stored accumulator (the RESUME instantiation)
  a 1/8 row share    the pipelined small share, which sums in-kernel without being asked to"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import material_scenes as ms
import oracle.binding as orc
import raytracingc_amd as rt
from chain_path_scenes import CHUNK_CLUSTERS, SCENES as BOX_SCENES, WGS_HIT_SHARE, clusters_of, prim_f_staged
from conftest import load_tris
from test_gpu_chain_paths import ROUTES, check_report, compare, expected_report

pytestmark = pytest.mark.gpu

W, H, MAX_BOUNCE = 96, 54, 10
INLINE_ROUTES = ("joined_inline", "pipelined_inline")
GOLDEN = ("ultracomplex", "fsuzane")
BOXES = ("box_gloss", "box_diffuse_T")
# one finite frame; -0 colours; emission 3e38 (inf, and inf - inf = NaN across samples); NaN, +inf and -inf materials in a
# closed and in an open scene (spp and maxBounce as material_scenes.FRAMES has them: more would leave only NaN pixels)
MATERIAL_FRAMES = ("cbox_bright", "cbox_zero", "cbox_blinding", "cbox_nonfinite", "copen_nonfinite")
ODD_SPP = (1, 2, 3, 5, 63, 65, 130)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(triangles, camera, note) as tests/chain_path_scenes.py's SCENES holds them; the golden models under the default
    camera, hit-heavy by the upload's own probe."""
    if name in GOLDEN:
        tris = load_tris(name)[0]
        tris.setflags(write=False)
        heavy = rt.bounce_hit_share(tris) > WGS_HIT_SHARE
        return tris, rt.camera_basis(), f"{name}: golden model; {'hit-heavy' if heavy else 'not hit-heavy'}"
    return BOX_SCENES[name] if name in BOX_SCENES else ms.SCENES[name]


@functools.lru_cache(maxsize=None)
def _device_scene(name):
    return rt.DeviceScene(_scene(name)[0], None)


@functools.lru_cache(maxsize=None)
def _oracle(name, sky_frame, width, height, spp, mb, row_start=0, row_stride=1):
    """The oracle's (u8, floats, segments), computed once and left unchanged."""
    tris, cam, _ = _scene(name)
    d = rt.RenderConfig(width, height, spp, mb, True, row_start=row_start, row_stride=row_stride).desc()
    col, acc, seg = orc.render(tris, None, _sky(sky_frame), cam, d, threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


def _sky(sky_frame):
    return ms.sky(sky_frame) if sky_frame else rt.default_scene()


def _summed_in_kernel(ds, before, name, route, counters, what, resume=False, small_share=False):
    """The launch ran, and no item of it had a deferred slot."""
    if name in GOLDEN:
        rep = ds.chain_report()
        assert rep["launches"] == before["launches"] + 1, f"{what}: no geometry-kernel launch"
        ncl = clusters_of(len(_scene(name)[0]))
        general = (ncl > CHUNK_CLUSTERS or counters or resume or not prim_f_staged(len(_scene(name)[0]), rep["wgs_per_cu"]))
        assert (rep["general"], rep["count"], rep["resume"], rep["spheres"]) == (general, counters, resume, False), \
            f"{what}: the launch ran {rep}"
        assert rep["chain_prim_f"] or ncl > CHUNK_CLUSTERS, f"{what}: unstaged filter records sum deferred"
        if name == "ultracomplex":  # the benchmark's scene: the kernel without the GENERAL code
            assert rep["general"] == (counters or resume) and not rep["multi"] and not rep["hits"], f"{what}: {rep}"
        return
    want = expected_report(name, route, counters, resume=resume, small_share=small_share,
                           scenes={name: _scene(name)})
    assert want["chain_prim_f"], f"{what}: unstaged filter records sum deferred"
    check_report(ds, before, want, what)


def _render_both(name, route, width, height, spp, mb, sky_frame=None, rows=None):
    """The launch without and with segment counters (the kernel without the GENERAL code where the scene allows it, then
    the counting GENERAL one: both sum in-kernel), each against the oracle."""
    import torch

    kw = dict(ROUTES[route])
    small_share = rows is not None
    if small_share:
        kw.update(row_start=rows[0], row_stride=rows[1])
    cfg = rt.RenderConfig(width, height, spp, mb, True, **kw)
    ocol, oacc, oseg = _oracle(name, sky_frame, width, height, spp, mb, *(rows or ()))
    ds = _device_scene(name)
    st = torch.cuda.current_stream().cuda_stream
    for counters in (False, True):
        out = torch.zeros((cfg.rows(), width, 3), dtype=torch.uint8, device="cuda")
        acc = torch.zeros((cfg.rows(), width, 3), dtype=torch.float32, device="cuda")
        seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
        torch.cuda.synchronize()
        before = ds.chain_report()
        ds.render_rows_async(_sky(sky_frame), _scene(name)[1], cfg, out.data_ptr(), acc.data_ptr(),
                             seg.data_ptr() if counters else None, st)
        torch.cuda.synchronize()
        what = f"{name} {width}x{height}x{spp} {route} rows={rows} counters={counters}"
        _summed_in_kernel(ds, before, name, route, counters, what, small_share=small_share)
        compare(what, out.cpu().numpy(), acc.cpu().numpy(), ocol, oacc)
        if counters:
            assert int(seg.cpu().numpy()[0]) == oseg, f"{what}: segments"


@pytest.mark.parametrize("route", INLINE_ROUTES)
def test_one_full_window(route, gpu_available):
    """ultracomplex, 64 samples: every item one window of 64 staged samples, the unrolled body."""
    _render_both("ultracomplex", route, W, H, 64, MAX_BOUNCE)


@pytest.mark.parametrize("route", INLINE_ROUTES)
@pytest.mark.parametrize("spp", ODD_SPP)
def test_partial_quads_and_several_windows(spp, route, gpu_available):
    _render_both("ultracomplex", route, W, H, spp, MAX_BOUNCE)


@pytest.mark.parametrize("route", INLINE_ROUTES)
@pytest.mark.parametrize("name", ("fsuzane",) + BOXES)
def test_interrupted_runs_and_mid_window_flushes(name, route, gpu_available):
    """Samples with h != 1: single-lane staging between the runs; fsuzane's geometry pixels whose primary ray misses flush
    mid-window and stage again.  The boxes are closed: every sample of theirs has several hits."""
    _render_both(name, route, W, H, 64, MAX_BOUNCE)


@pytest.mark.parametrize("route", INLINE_ROUTES)
@pytest.mark.parametrize("frame", MATERIAL_FRAMES)
def test_nonfinite_and_signed_zero_samples(frame, route, gpu_available):
    name, _, _, spp, mb = ms.FRAMES[frame]
    _, oacc, _ = _oracle(name, frame, W, H, spp, mb)
    if frame in ms.NAN_FRAMES:  # the frame holds what it is here for, beside pixels a wrong sum would change
        assert np.isnan(oacc).any() and (np.isinf(oacc).any() or frame.endswith("_nonfinite")) and np.isfinite(oacc).any()
    elif frame == "cbox_zero":
        assert (oacc == 0).any() and np.isfinite(oacc).all()
    else:
        assert np.isfinite(oacc).all()
    _render_both(name, route, W, H, spp, mb, sky_frame=frame)


@pytest.mark.parametrize("name", ("ultracomplex", "box_diffuse_T"))
def test_two_passes_equal_one_launch(name, gpu_available):
    """16 + 48 samples through rtc_render_samples_async, summing in-kernel: the second pass starts from the stored
    accumulator.  The buffers are filled with 0xFF bytes first; afterwards they are one 64-sample launch's and the oracle's."""
    import torch

    tris, cam, _ = _scene(name)
    scene = rt.default_scene()
    cfg = rt.RenderConfig(W, H, 64, MAX_BOUNCE, True, **ROUTES["joined_inline"])
    ocol, oacc, oseg = _oracle(name, None, W, H, 64, MAX_BOUNCE)
    ds = _device_scene(name)
    st = torch.cuda.current_stream().cuda_stream
    one = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    one_acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    ds.render_rows_async(scene, cam, cfg, one.data_ptr(), one_acc.data_ptr(), None, st)
    for counters in (False, True):
        col = torch.full((H, W, 3), 0xFF, dtype=torch.uint8, device="cuda")
        acc = torch.full((H, W, 3), -1, dtype=torch.int32, device="cuda")  # 0xFF bytes
        rng = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
        done = 0
        for count in (16, 48):
            torch.cuda.synchronize()
            before = ds.chain_report()
            ds.render_samples_async(scene, cam, cfg, done, count, col.data_ptr(), acc.data_ptr(), rng.data_ptr(),
                                    seg.data_ptr() if counters else None, st)
            torch.cuda.synchronize()
            done += count
            _summed_in_kernel(ds, before, name, "joined_inline", counters, f"{name} pass to {done} counters={counters}",
                              resume=True)
        what = f"{name} 16 + 48 counters={counters}"
        a = acc.cpu().numpy().view(np.float32)
        compare(what, col.cpu().numpy(), a, ocol, oacc)
        assert np.array_equal(a.view(np.uint32), one_acc.cpu().numpy().view(np.uint32)), f"{what}: one launch's floats"
        assert np.array_equal(col.cpu().numpy(), one.cpu().numpy()), f"{what}: one launch's bytes"
        if counters:
            assert int(seg.cpu().numpy()[0]) == oseg, f"{what}: segments"


@pytest.mark.parametrize("rank", (0, 5))
def test_pipelined_row_share(rank, gpu_available):
    """Rows y = rank + 8 k of a 96x432 frame, pipelined without RTC_F_CHAIN_INLINE: the small-share route, which takes the
    in-kernel sums by default."""
    _render_both("ultracomplex", "pipelined", W, 8 * H, 64, MAX_BOUNCE, rows=(rank, 8))
