"""rtc_occluded_async / rtc_occluded at the C ABI (include/rtc.h): the symbols, the Python surface, the flag's
value and the refusals that come before any device call and before the scene handle is read, so they hold without a GPU (a
fake handle that is never dereferenced stands in for a scene); and that no entry point takes 0x8000, the bit of the
deleted RTC_F_NO_REACH_CULL.  The values are tests/test_gpu_occluded.py's business.  Reference seam:
calculateRayCollision(Ray ray, int trianglesOnly) (raytracing.c:216-240)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import raytracingc_amd as rt
from raytracingc_amd import _abi
from raytracingc_amd._abi import RTC_EINVAL, RTC_ENODEV, RtcHitBuffers, RtcPathDesc

FAKE = C.c_void_p(0x10)      # a scene handle that must never be dereferenced
RAYS = C.c_void_p(0x2000)    # nor these "device" buffers
TMAX = C.c_void_p(0x3000)
OCC = C.c_void_p(0x4001)     # (any byte alignment)
COUNT = C.c_void_p(0x5000)
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
NO_REACH = 0x8000  # the bit of the deleted RTC_F_NO_REACH_CULL: no entry point takes it


def _msg():
    return rt.lib().rtc_last_error()


def test_symbols_and_python_surface():
    L = rt.lib()
    names = {"rtc_occluded_async", "rtc_occluded", "rtc_plan_sim_occluded"}
    assert all(hasattr(L, n) for n in names) and names <= set(_abi.EXPORTS)
    assert hasattr(rt.DeviceScene, "occluded_async") and hasattr(rt.DeviceScene, "occluded")
    assert NO_CULL == 0x20 and not hasattr(rt, "RTC_F_NO_REACH_CULL") and not hasattr(_abi, "RTC_F_NO_REACH_CULL")


def test_async_refusals_come_before_any_device_call():
    L = rt.lib()
    f = L.rtc_occluded_async
    assert f(None, RAYS, TMAX, 4, 0, 0, OCC, COUNT, None) == RTC_EINVAL
    assert b"rtc_occluded_async" in _msg() and b"null scene" in _msg()
    assert f(FAKE, None, TMAX, 4, 0, 0, OCC, COUNT, None) == RTC_EINVAL
    assert b"rtc_occluded_async" in _msg() and b"null" in _msg()
    for tmax in (TMAX, None):
        assert f(FAKE, RAYS, tmax, 4, 0, 0, None, None, None) == RTC_EINVAL
        assert b"rtc_occluded_async" in _msg() and b"no output" in _msg()
    for n in (0x80000000, 1 << 40):
        assert f(FAKE, RAYS, TMAX, n, 0, 0, OCC, None, None) == RTC_EINVAL
        assert b"rtc_occluded_async" in _msg() and b"rays" in _msg()
    for flags in (rt.RTC_F_NO_TILE_CULL, rt.RTC_F_OVERLAP, NO_CULL | rt.RTC_F_HOIST_PRIMARY, NO_REACH, NO_REACH | NO_CULL,
                  0x10000, 0x40000000):
        assert f(FAKE, RAYS, None, 4, 1, flags, None, COUNT, None) == RTC_EINVAL
        assert b"rtc_occluded_async" in _msg() and b"flags" in _msg()


@pytest.mark.parametrize("flags", [0, NO_CULL])
def test_no_rays_is_fine_and_enqueues_nothing(flags):
    """n == 0 returns 0 before the handle is read, under every flag the entry takes and every nullable combination; the
    refusals still come first."""
    f = rt.lib().rtc_occluded_async
    assert f(FAKE, RAYS, TMAX, 0, 0, flags, OCC, COUNT, None) == 0
    assert f(FAKE, RAYS, None, 0, 1, flags, OCC, None, None) == 0
    assert f(FAKE, RAYS, None, 0, 1, flags, None, COUNT, None) == 0
    assert f(FAKE, RAYS, None, 0, 0, flags | rt.RTC_F_OVERLAP, OCC, None, None) == RTC_EINVAL
    assert f(None, RAYS, None, 0, 0, flags, OCC, None, None) == RTC_EINVAL
    assert f(FAKE, RAYS, None, 0, 0, flags, None, None, None) == RTC_EINVAL


def test_host_entry_has_the_same_refusals():
    L = rt.lib()
    rays, lim, occ = np.zeros(4, _abi.RAY_DT), np.ones(4, np.float32), np.zeros(4, np.uint8)
    cnt = C.c_ulonglong(0)
    rp, tp, op = (a.ctypes.data_as(C.c_void_p) for a in (rays, lim, occ))
    cp = C.cast(C.pointer(cnt), C.c_void_p)
    f = L.rtc_occluded
    assert f(None, rp, tp, 4, 0, 0, op, cp) == RTC_EINVAL
    assert b"rtc_occluded:" in _msg() and b"null scene" in _msg()
    assert f(FAKE, None, tp, 4, 0, 0, op, cp) == RTC_EINVAL
    assert b"rtc_occluded:" in _msg() and b"null" in _msg()
    assert f(FAKE, rp, tp, 4, 0, 0, None, None) == RTC_EINVAL
    assert b"rtc_occluded:" in _msg() and b"no output" in _msg()
    assert f(FAKE, rp, tp, 1 << 31, 0, 0, op, cp) == RTC_EINVAL
    assert f(FAKE, rp, tp, 4, 0, rt.RTC_F_NO_COOP, op, cp) == RTC_EINVAL
    assert b"rtc_occluded:" in _msg() and b"flags" in _msg()
    assert f(FAKE, rp, None, 0, 0, NO_REACH, op, None) == RTC_EINVAL
    assert f(FAKE, rp, None, 0, 0, NO_CULL, op, None) == 0
    assert cnt.value == 0 and not occ.any()


def test_host_entry_without_a_gpu_is_enodev():
    """Without a device the host entry returns RTC_ENODEV before it reads the handle (with one, the fake handle cannot be
    used: the GPU tests cover the entry)."""
    if rt.device_count() > 0:
        return  # (tests/test_gpu_occluded.py runs the host entry on a real scene)
    rays, occ = np.zeros(4, _abi.RAY_DT), np.zeros(4, np.uint8)
    assert rt.lib().rtc_occluded(FAKE, rays.ctypes.data_as(C.c_void_p), None, 4, 0, 0, occ.ctypes.data_as(C.c_void_p),
                                 None) == RTC_ENODEV


def test_the_other_entry_points_refuse_the_flag():
    """0x8000 is no flag of the ray, path and first-hit entries either: they whitelist their flags."""
    L = rt.lib()
    out = RtcHitBuffers(C.c_void_p(0x1000), None, None, None)
    for flags in (NO_REACH, NO_REACH | NO_CULL):
        assert L.rtc_trace_rays_async(FAKE, RAYS, 4, 0, flags, C.byref(out), None) == RTC_EINVAL
        assert b"rtc_trace_rays_async" in _msg() and b"flags" in _msg()
        d = RtcPathDesc(4, 2, 1, flags, 0, 4)
        assert L.rtc_trace_paths_async(FAKE, C.byref(rt.default_scene()), RAYS, C.c_void_p(0x6000), 4, C.byref(d),
                                       C.c_void_p(0x7000), None, None, None) == RTC_EINVAL
        assert b"rtc_trace_paths_async" in _msg() and b"flags" in _msg()
    # the first-hit entry checks its flags while it plans the launch, so on the planner's hook (no scene is read there)
    sim = C.c_void_p()
    assert L.rtc_plan_sim_create(120, 0, C.byref(sim)) == 0
    try:
        ops, fp = (C.c_int * 256)(), (C.c_ulonglong * 1536)()
        d = rt.RenderConfig(64, 40, 0, 0, True).desc()
        cam, env = (C.c_float * 13)(), (C.c_float * 14)()
        for flags in (NO_REACH, NO_REACH | rt.RTC_F_NO_TILE_CULL):
            d.flags = flags
            assert L.rtc_plan_sim_set_first_hit(sim, 0x1000, 0, 0, 0) == 0
            assert L.rtc_plan_sim_launch(sim, C.byref(d), 0, 0, 0, 0, cam, env, ops, 64, fp, 256) == RTC_EINVAL
        hit = (C.c_ulonglong * 4)(0x1000, 0, 0, 0)
        assert L.rtc_plan_sim_trace_rays(sim, 0, 0x2000, hit, NO_REACH, ops, 64, fp, 256) == RTC_EINVAL
        assert L.rtc_plan_sim_trace_paths(sim, 0, 0x2000, 0x6000, 0x7000, 0, 0, 0, NO_REACH, ops, 64, fp, 256) == RTC_EINVAL
    finally:
        L.rtc_plan_sim_release(sim)


def test_python_arguments_are_checked():
    ds = rt.DeviceScene.__new__(rt.DeviceScene)  # (no upload: the argument checks come first)
    ds._h = None
    with pytest.raises(ValueError):
        ds.occluded(np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError):
        ds.occluded(np.zeros((2, 6), np.float32), tmax=np.ones(3, np.float32))
    with pytest.raises(ValueError):
        ds.occluded(np.zeros(2, _abi.RAY_DT), tmax=np.ones((2, 2), np.float32))
    got = ds.occluded(np.zeros((0, 6), np.float32))
    assert got.shape == (0,) and got.dtype == bool
    got, n = ds.occluded(np.zeros(0, _abi.RAY_DT), tmax=1.0, count=True)
    assert got.shape == (0,) and got.dtype == bool and n == 0
