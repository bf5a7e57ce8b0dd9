"""RTC_F_WAVE_PER_RAY at the C ABI (include/rtc.h), without a GPU: the constant, which entries take it -- the
path query's two, alone or with RTC_F_NO_CLUSTER_CULL -- and which refuse it, before any device call and before the scene
handle is read (a fake handle that is never dereferenced stands in for a scene); and that the planner plans the same
operation and the same footprint records with and without it.  The values are tests/test_gpu_trace_paths_wave.py's
business.  No reference counterpart (the flag selects a kernel, never a value)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import raytracingc_amd as rt
from raytracingc_amd import _abi
from raytracingc_amd._abi import RTC_EINVAL, RtcHitBuffers, RtcPathDesc

FAKE = C.c_void_p(0x10)      # a scene handle that must never be dereferenced
RAYS = C.c_void_p(0x2000)    # nor these "device" buffers
SEEDS = C.c_void_p(0x3000)
RAD = C.c_void_p(0x4000)
WAVE = rt.RTC_F_WAVE_PER_RAY
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
SCENE = rt.default_scene()


def _msg():
    return rt.lib().rtc_last_error()


def _paths(flags, n=0):
    d = RtcPathDesc(4, 10, 0, flags, 0, 4)
    return rt.lib().rtc_trace_paths_async(FAKE, C.byref(SCENE), RAYS, SEEDS, n, C.byref(d), RAD, None, None, None)


def test_the_constant():
    assert WAVE == 0x20000 and _abi.RTC_F_WAVE_PER_RAY == 0x20000
    others = [getattr(_abi, k) for k in dir(_abi) if k.startswith("RTC_F_") and k != "RTC_F_WAVE_PER_RAY"]
    assert all(WAVE & v == 0 for v in others)
    assert WAVE not in (0x8000, 0x10000, 0x40000000)  # bits other tests pin as refused everywhere


def test_the_path_query_takes_it():
    """n == 0 returns 0 before the handle is read; the other refusals still come first."""
    assert _paths(WAVE) == 0
    assert _paths(WAVE | NO_CULL) == 0
    for flags in (WAVE | rt.RTC_F_OVERLAP, WAVE | rt.RTC_F_DEBUG_BOUNCES):
        assert _paths(flags) == RTC_EINVAL
        assert b"rtc_trace_paths_async" in _msg() and b"flags" in _msg()
        assert _paths(flags, 4) == RTC_EINVAL


def test_the_host_entry_takes_it():
    rays, seeds, rad = np.zeros(4, _abi.RAY_DT), np.zeros(4, np.uint32), np.zeros((4, 3), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for flags, want in ((WAVE, 0), (WAVE | NO_CULL, 0), (WAVE | rt.RTC_F_NO_TILE_CULL, RTC_EINVAL)):
        d = RtcPathDesc(4, 10, 0, flags, 0, 4)
        assert rt.lib().rtc_trace_paths(FAKE, C.byref(SCENE), p(rays), p(seeds), 0, C.byref(d), p(rad), None, None) == want


def test_the_other_entry_points_refuse_it():
    L = rt.lib()
    out = RtcHitBuffers(C.c_void_p(0x1000), None, None, None)
    occ = C.c_void_p(0x5000)
    for flags in (WAVE, WAVE | NO_CULL):
        for n in (0, 4):
            assert L.rtc_trace_rays_async(FAKE, RAYS, n, 0, flags, C.byref(out), None) == RTC_EINVAL
            assert b"rtc_trace_rays_async" in _msg() and b"flags" in _msg()
            assert L.rtc_occluded_async(FAKE, RAYS, None, n, 0, flags, occ, None, None) == RTC_EINVAL
            assert b"rtc_occluded_async" in _msg() and b"flags" in _msg()
    # the first-hit entry checks its flags while it plans the launch, so on the planner's hook (no scene is read there)
    sim = C.c_void_p()
    assert L.rtc_plan_sim_create(120, 0, C.byref(sim)) == 0
    try:
        ops, fp = (C.c_int * 256)(), (C.c_ulonglong * 1536)()
        d = rt.RenderConfig(64, 40, 0, 0, True).desc()
        cam, env = (C.c_float * 13)(), (C.c_float * 14)()
        for flags in (WAVE, WAVE | rt.RTC_F_NO_TILE_CULL):
            d.flags = flags
            assert L.rtc_plan_sim_set_first_hit(sim, 0x1000, 0, 0, 0) == 0
            assert L.rtc_plan_sim_launch(sim, C.byref(d), 0, 0, 0, 0, cam, env, ops, 64, fp, 256) == RTC_EINVAL
        hit = (C.c_ulonglong * 4)(0x1000, 0, 0, 0)
        assert L.rtc_plan_sim_trace_rays(sim, 0, 0x2000, hit, WAVE, ops, 64, fp, 256) == RTC_EINVAL
        assert L.rtc_plan_sim_occluded(sim, 0, 0x2000, 0, 0x5000, 0, WAVE, ops, 64, fp, 256) == RTC_EINVAL
    finally:
        L.rtc_plan_sim_release(sim)


def _plan(sim, flags, seeds_out, segments, first):
    ops, fp = (C.c_int * 256)(), (C.c_ulonglong * 1536)()
    rc = rt.lib().rtc_plan_sim_trace_paths(sim, 0x7f001000, 0x2000, 0x6000, 0x7000, seeds_out, segments, first, flags, ops,
                                           64, fp, 256)
    if rc <= 0:
        return rc, None, None
    nops, nfp = rc & 0xFF, rc >> 8
    return rc, list(ops[:4 * nops]), list(fp[:6 * nfp])


def test_the_planner_plans_the_same_operation():
    """Kernel 12 on the caller's stream with paths_footprint's rows, whatever the outputs asked for."""
    L = rt.lib()
    sim = C.c_void_p()
    assert L.rtc_plan_sim_create(300, 0, C.byref(sim)) == 0
    try:
        for seeds_out, segments, first in ((0, 0, 0), (0x6000, 0, 0), (0x8000, 0x9000, 0), (0x6000, 0x9000, 3)):
            base = _plan(sim, 0, seeds_out, segments, first)
            assert base[0] > 0 and base[1][3] == 12 and len(base[1]) == 4
            for flags, ref in ((WAVE, base), (WAVE | NO_CULL, _plan(sim, NO_CULL, seeds_out, segments, first))):
                assert _plan(sim, flags, seeds_out, segments, first) == ref == base
        for flags in (WAVE | rt.RTC_F_NO_TILE_CULL, WAVE | rt.RTC_F_OVERLAP, WAVE | 0x40000000):
            assert _plan(sim, flags, 0, 0, 0)[0] == RTC_EINVAL
    finally:
        L.rtc_plan_sim_release(sim)
