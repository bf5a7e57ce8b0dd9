"""Whole frames of the chain-path scenes (tests/chain_path_scenes.py: 16, 17, 32 and 33 clusters, hit-heavy boxes of 18, 20
and 21 clusters, maxBounce 40 to 100) on every route of the renderer, against the CPU oracle: NaN positions equal, every
other float of the accumulator bit-equal, the u8 frame equal, the segment count equal where the launch counts -- bit
comparisons, no tolerance.  The routes are those of tests/test_gpu_adversarial_frames.py and the pipelined launch that sums
in-kernel (at these frame sizes the one pipelined whole frame without deferred slots) and the in-kernel sums without the
cluster cull, each with and without segment counters; three scenes also as two passes split inside a window (rtc_render_samples_async), whose RNG states are the
progressive reference's.

Every choice of rtc_render_chain's renders the same frame, so after each launch DeviceScene.chain_report (host state
recorded by the launch code) is compared with what the launch was meant to run: the kernel without the GENERAL code for the
in-kernel sums, its HITS instantiation for the hit-heavy boxes, a GENERAL kernel reading the primary filter records from
global memory for box_primf_4 and staged ones for its neighbour, MULTI for 33 clusters.  What the lanes and clusters then
do inside the kernel follows from the oracle alone (tests/test_chain_path_scenes.py)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import progressive_reference as pr
import raytracingc_amd as rt
from chain_path_scenes import (CHAIN_STATIC_LDS, CHUNK_CLUSTERS, CU_LDS, FRAMES, PASS_FRAMES, PASS_SPLIT, SCENES, clusters_of,
                               prim_f_staged)
from test_gpu_adversarial_frames import ROUTES as ADVERSARIAL_ROUTES

pytestmark = pytest.mark.gpu

ROUTES = dict(ADVERSARIAL_ROUTES, pipelined_inline=dict(overlap=True, chain_inline=True),
              inline_no_cluster_cull=dict(chain_inline=True, cluster_cull=False))
NO_GEOMETRY_KERNEL = ("no_tile_cull", "no_coop")  # launches without the split launch: the report stays as it was
# no deferred slots: the kernels without the GENERAL code (without the cluster cull: their per-lane build and its flush)
IN_KERNEL_SUMS = ("joined_inline", "pipelined_inline", "inline_no_cluster_cull")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hit_heavy(scene_name, scenes=SCENES):
    return "not hit-heavy" not in scenes[scene_name][2]  # (tests/test_chain_path_scenes.py holds the notes to the probe)


@functools.lru_cache(maxsize=None)
def _oracle(scene_name, W, H, spp, mb, row_start=0, row_stride=1):
    """The oracle's (u8, floats, segments) of the frame, computed once and left unchanged."""
    tris, cam, _ = SCENES[scene_name]
    d = rt.RenderConfig(W, H, spp, mb, True, row_start=row_start, row_stride=row_stride).desc()
    col, acc, seg = orc.render(tris, None, rt.default_scene(), cam, d, threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


@functools.lru_cache(maxsize=None)
def _device_scene(scene_name):
    return rt.DeviceScene(SCENES[scene_name][0], None)


def expected_report(scene_name, route, counters, resume=False, small_share=False, scenes=SCENES):
    """What run_chain / size_chain_lds choose for this launch (rtc_render.hip), from the scene's size and hit share;
    `scenes`: another table of the same form (tests/material_scenes.py's)."""
    T = len(scenes[scene_name][0])
    ncl = clusters_of(T)
    multi = ncl > CHUNK_CLUSTERS
    wgs = 3 if small_share or not _hit_heavy(scene_name, scenes) else 4
    staged = prim_f_staged(T, wgs)
    in_kernel = route in IN_KERNEL_SUMS or small_share
    defer = not in_kernel or route == "hoisted" or not staged
    general = multi or counters or defer or resume
    return dict(multi=multi, count=counters, hits=_hit_heavy(scene_name, scenes) and not general, general=general, spheres=False,
                resume=resume, chain_prim_f=staged, wgs_per_cu=wgs, cluster_count=ncl,
                chunk_count=(ncl + CHUNK_CLUSTERS - 1) // CHUNK_CLUSTERS)


def check_report(ds, before, want, what):
    rep = ds.chain_report()
    assert rep["launches"] == before["launches"] + 1, f"{what}: no geometry-kernel launch"
    got = {k: rep[k] for k in want}
    assert got == want, f"{what}: the launch ran {got}, meant {want}"
    # the dynamic LDS: the records (single chunk), the staged filter records, at least the floor that keeps the per-CU count
    ncl = want["cluster_count"]
    need = (0 if want["multi"] else 512 * ncl) + (512 * ncl if want["chain_prim_f"] else 0)
    assert rep["chain_dyn"] >= need and rep["chain_dyn"] + CHAIN_STATIC_LDS <= CU_LDS // want["wgs_per_cu"], what
    return rep


def compare(what, col, a, ocol, oacc):
    nan = np.isnan(oacc)
    assert np.array_equal(np.isnan(a), nan), f"{what}: NaN positions differ ({int(np.isnan(a).sum())} vs {int(nan.sum())})"
    bad = int(((_bits(a) != _bits(oacc)) & ~nan).any(-1).sum())
    assert bad == 0, f"{what}: {bad} pixels' accumulator bits differ"
    assert np.array_equal(col, ocol), f"{what}: {int((col != ocol).any(-1).sum())} u8 pixels differ"


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_frame_matches_oracle(frame, route, gpu_available):
    import torch

    scene_name, W, H, spp, mb = FRAMES[frame]
    cam = SCENES[scene_name][1]
    scene = rt.default_scene()
    cfg = rt.RenderConfig(W, H, spp, mb, True, **ROUTES[route])
    ocol, oacc, oseg = _oracle(scene_name, W, H, spp, mb)
    ds = _device_scene(scene_name)
    st = torch.cuda.current_stream().cuda_stream
    # the route itself (a launch that counts segments is always a joined one), then the same launch counting
    for counters in (False, True):
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
        torch.cuda.synchronize()
        before = ds.chain_report()
        ds.render_rows_async(scene, cam, cfg, out.data_ptr(), acc.data_ptr(), seg.data_ptr() if counters else None, st)
        torch.cuda.synchronize()
        what = f"{frame} {route} counters={counters}"
        if route in NO_GEOMETRY_KERNEL:
            assert ds.chain_report() == before, what
        else:
            check_report(ds, before, expected_report(scene_name, route, counters), what)
        compare(what, out.cpu().numpy(), acc.cpu().numpy(), ocol, oacc)
        if counters:
            assert int(seg.cpu().numpy()[0]) == oseg, f"{what}: segments"


def test_small_share_of_box_primf_4_is_staged(gpu_available):
    """The same 21-cluster scene as a small row share runs 3 workgroups per CU, where its primary filter records fit:
    staged, so the pipelined share runs the HITS kernel -- no GENERAL code -- at 21 clusters; the rows are the oracle's."""
    import torch

    scene_name, W, H, spp, mb = FRAMES["box_primf_4"]
    cam, scene = SCENES[scene_name][1], rt.default_scene()
    cfg = rt.RenderConfig(W, H, spp, mb, True, overlap=True, row_start=1, row_stride=2)
    ocol, oacc, _ = _oracle(scene_name, W, H, spp, mb, 1, 2)
    ds = _device_scene(scene_name)
    out = torch.zeros((cfg.rows(), W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((cfg.rows(), W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = ds.chain_report()
    ds.render_rows_async(scene, cam, cfg, out.data_ptr(), acc.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = expected_report(scene_name, "pipelined", False, small_share=True)
    assert want["chain_prim_f"] and want["wgs_per_cu"] == 3 and want["hits"] and not want["general"]
    check_report(ds, before, want, "box_primf_4 rows 1+2k")
    compare("box_primf_4 rows 1+2k", out.cpu().numpy(), acc.cpu().numpy(), ocol, oacc)


# ---- two passes, split inside a window -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pass_reference(frame):
    scene_name, W, H, mb = PASS_FRAMES[frame]
    tris, cam, _ = SCENES[scene_name]
    d = rt.RenderConfig(W, H, sum(PASS_SPLIT), mb, True).desc()
    ch = pr.chain(tris, None, rt.default_scene(), cam, d, list(PASS_SPLIT), {})
    for t in ch:
        for a in t[1:4]:
            a.setflags(write=False)
    return ch


@pytest.mark.parametrize("route", ["joined_deferred", "joined_inline", "hoisted"])
@pytest.mark.parametrize("frame", sorted(PASS_FRAMES))
def test_two_passes_match_the_reference(frame, route, gpu_available):
    import torch

    scene_name, W, H, mb = PASS_FRAMES[frame]
    cam, scene = SCENES[scene_name][1], rt.default_scene()
    spp = sum(PASS_SPLIT)
    cfg = rt.RenderConfig(W, H, spp, mb, True, **ROUTES[route])
    ch = _pass_reference(frame)
    ocol, oacc, oseg = _oracle(scene_name, W, H, spp, mb)
    ds = _device_scene(scene_name)
    st = torch.cuda.current_stream().cuda_stream
    for counters in (False, True):
        col = torch.full((H, W, 3), 0xFF, dtype=torch.uint8, device="cuda")
        acc = torch.full((H, W, 3), -1, dtype=torch.int32, device="cuda")  # 0xFF bytes
        rng = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
        done = 0
        for count, (rdone, racc, rrng, rcol, _) in zip(PASS_SPLIT, ch):
            torch.cuda.synchronize()
            before = ds.chain_report()
            ds.render_samples_async(scene, cam, cfg, done, count, col.data_ptr(), acc.data_ptr(), rng.data_ptr(),
                                    seg.data_ptr() if counters else None, st)
            torch.cuda.synchronize()
            done += count
            what = f"{frame} {route} counters={counters} after {done}/{spp}"
            check_report(ds, before, expected_report(scene_name, route, counters, resume=True), what)
            a, s, c = acc.cpu().numpy().view(np.uint32), rng.cpu().numpy().view(np.uint32), col.cpu().numpy()
            bad = int((a != _bits(racc)).sum()), int((s != rrng).sum()), int((c != rcol).sum())
            assert done == rdone and bad == (0, 0, 0), f"{what}: differing accumulator words, states, colour bytes {bad}"
        compare(f"{frame} {route} counters={counters}: the oracle's frame", c, a.view(np.float32), ocol, oacc)
        if counters:
            assert int(seg.cpu().numpy()[0]) == oseg, f"{frame} {route}: segments"
