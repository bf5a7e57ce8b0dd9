"""rtc_trace_rays_async / rtc_trace_rays at the C ABI (include/rtc.h): the symbols, the Python surface and the
refusals that come before any device call and before the scene handle is read, so they hold without a GPU (a fake handle
that is never dereferenced stands in for a scene).  The values are tests/test_gpu_trace_rays.py's business.  Reference
seam: calculateRayCollision(Ray ray, int trianglesOnly) (raytracing.c:216-240)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import raytracingc_amd as rt
from raytracingc_amd import _abi
from raytracingc_amd._abi import RTC_EINVAL, RTC_ENODEV, RtcHitBuffers

FAKE = C.c_void_p(0x10)      # a scene handle that must never be dereferenced
RAYS = C.c_void_p(0x2000)    # nor this "device" ray buffer
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL


def _out(*ptrs):
    return RtcHitBuffers(*[C.c_void_p(p) if p else None for p in ptrs])


def _msg():
    return rt.lib().rtc_last_error()


def test_symbols_and_python_surface():
    L = rt.lib()
    names = {"rtc_trace_rays_async", "rtc_trace_rays", "rtc_plan_sim_trace_rays"}
    assert all(hasattr(L, n) for n in names) and names <= set(_abi.EXPORTS)
    assert hasattr(rt.DeviceScene, "trace_rays_async") and hasattr(rt.DeviceScene, "trace_rays")
    assert NO_CULL == 0x20 and _abi.RAY_DT.itemsize == 24


def test_async_refusals_come_before_any_device_call():
    L = rt.lib()
    out = _out(0x1000, 0, 0, 0)
    assert L.rtc_trace_rays_async(None, RAYS, 4, 0, 0, C.byref(out), None) == RTC_EINVAL
    assert b"rtc_trace_rays_async" in _msg() and b"null scene" in _msg()
    assert L.rtc_trace_rays_async(FAKE, None, 4, 0, 0, C.byref(out), None) == RTC_EINVAL
    assert b"rtc_trace_rays_async" in _msg() and b"null" in _msg()
    assert L.rtc_trace_rays_async(FAKE, RAYS, 4, 0, 0, None, None) == RTC_EINVAL
    assert b"rtc_trace_rays_async" in _msg() and b"null" in _msg()
    none = _out(0, 0, 0, 0)
    assert L.rtc_trace_rays_async(FAKE, RAYS, 4, 0, 0, C.byref(none), None) == RTC_EINVAL
    assert b"rtc_trace_rays_async" in _msg() and b"no buffer" in _msg()
    for n in (0x80000000, 1 << 40):
        assert L.rtc_trace_rays_async(FAKE, RAYS, n, 0, 0, C.byref(out), None) == RTC_EINVAL
        assert b"rtc_trace_rays_async" in _msg() and b"rays" in _msg()
    for flags in (rt.RTC_F_NO_TILE_CULL, rt.RTC_F_OVERLAP, NO_CULL | rt.RTC_F_HOIST_PRIMARY, 0x40000000):
        assert L.rtc_trace_rays_async(FAKE, RAYS, 4, 1, flags, C.byref(out), None) == RTC_EINVAL
        assert b"rtc_trace_rays_async" in _msg() and b"flags" in _msg()


def test_no_rays_is_fine_and_enqueues_nothing():
    """n == 0 returns 0 before the handle is read (with and without the brute-force flag); the refusals still come first."""
    L = rt.lib()
    out = _out(0x1000, 0x2000, 0, 0)
    assert L.rtc_trace_rays_async(FAKE, RAYS, 0, 0, 0, C.byref(out), None) == 0
    assert L.rtc_trace_rays_async(FAKE, RAYS, 0, 1, NO_CULL, C.byref(out), None) == 0
    assert L.rtc_trace_rays_async(FAKE, RAYS, 0, 0, rt.RTC_F_OVERLAP, C.byref(out), None) == RTC_EINVAL
    assert L.rtc_trace_rays_async(None, RAYS, 0, 0, 0, C.byref(out), None) == RTC_EINVAL


def test_host_entry_has_the_same_refusals():
    L = rt.lib()
    rays = np.zeros(4, _abi.RAY_DT)
    prim = np.zeros(4, np.int32)
    rp, pp = rays.ctypes.data_as(C.c_void_p), prim.ctypes.data_as(C.c_void_p)
    assert L.rtc_trace_rays(None, rp, 4, 0, 0, pp, None, None, None) == RTC_EINVAL
    assert b"rtc_trace_rays:" in _msg() and b"null scene" in _msg()
    assert L.rtc_trace_rays(FAKE, None, 4, 0, 0, pp, None, None, None) == RTC_EINVAL
    assert b"rtc_trace_rays:" in _msg() and b"null" in _msg()
    assert L.rtc_trace_rays(FAKE, rp, 4, 0, 0, None, None, None, None) == RTC_EINVAL
    assert b"rtc_trace_rays:" in _msg() and b"no buffer" in _msg()
    assert L.rtc_trace_rays(FAKE, rp, 1 << 31, 0, 0, pp, None, None, None) == RTC_EINVAL
    assert L.rtc_trace_rays(FAKE, rp, 4, 0, rt.RTC_F_NO_COOP, pp, None, None, None) == RTC_EINVAL
    assert b"rtc_trace_rays:" in _msg() and b"flags" in _msg()
    assert L.rtc_trace_rays(FAKE, rp, 0, 0, 0, pp, None, None, None) == 0


def test_host_entry_without_a_gpu_is_enodev():
    """Without a device the host entry returns RTC_ENODEV before it reads the handle (with one, the fake handle cannot be
    used: the GPU tests cover the entry)."""
    if rt.device_count() > 0:
        return  # (tests/test_gpu_trace_rays.py runs the host entry on a real scene)
    L = rt.lib()
    rays = np.zeros(4, _abi.RAY_DT)
    prim = np.zeros(4, np.int32)
    assert L.rtc_trace_rays(FAKE, rays.ctypes.data_as(C.c_void_p), 4, 0, 0, prim.ctypes.data_as(C.c_void_p), None, None,
                            None) == RTC_ENODEV


def test_python_want_is_checked():
    ds = rt.DeviceScene.__new__(rt.DeviceScene)  # (no upload: the argument check comes first)
    ds._h = None
    with pytest.raises(ValueError):
        ds.trace_rays(np.zeros((2, 6), np.float32), want=())
    with pytest.raises(ValueError):
        ds.trace_rays(np.zeros((2, 6), np.float32), want=("prim", "colour"))
    with pytest.raises(ValueError):
        ds.trace_rays(np.zeros((2, 5), np.float32))
    assert {k: v.shape for k, v in ds.trace_rays(np.zeros((0, 6), np.float32)).items()} == \
        {"prim": (0,), "depth": (0,), "normal": (0, 3), "albedo": (0, 3)}
