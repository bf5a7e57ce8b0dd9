"""rtc_ray_order_async / rtc_ray_order / rtc_gather_async / rtc_scatter_async at the C ABI (include/rtc.h): the
symbols, the Python surface, the scratch size, and the refusals that come before any device call and before the scene
handle is read, so they hold without a GPU (a fake handle that is never dereferenced stands in for a scene).  The values are
tests/test_gpu_ray_order.py's business."""
from __future__ import annotations

import ctypes as C
import inspect

import numpy as np
import pytest

import raytracingc_amd as rt
from raytracingc_amd import _abi
from raytracingc_amd._abi import RTC_EINVAL, RTC_ENODEV

FAKE = C.c_void_p(0x10)       # a scene handle that must never be dereferenced
RAYS = C.c_void_p(0x2000)     # nor these "device" buffers
ORDER = C.c_void_p(0x3000)
KEYS = C.c_void_p(0x4000)
SCRATCH = C.c_void_p(0x50000)
BIG = 1 << 40                 # "enough scratch" for any n the refusals use


def _msg():
    return rt.lib().rtc_last_error()


def test_symbols_and_python_surface():
    L = rt.lib()
    names = {"rtc_scene_bounds", "rtc_ray_order_shape", "rtc_ray_order_scratch_bytes", "rtc_ray_order_async", "rtc_ray_order", "rtc_ray_keys_host",
             "rtc_gather_async", "rtc_scatter_async"}
    assert all(hasattr(L, n) for n in names) and names <= set(_abi.EXPORTS)
    for f in ("ray_keys_host", "ray_order_scratch_bytes", "gather_async", "scatter_async"):
        assert callable(getattr(rt, f)) and f in rt.__all__
    for m in ("bounds", "ray_order", "ray_order_async"):
        assert hasattr(rt.DeviceScene, m)
    for m in ("trace_rays", "trace_paths", "occluded"):
        p = inspect.signature(getattr(rt.DeviceScene, m)).parameters
        assert "order" in p and p["order"].default is None, m


def test_sort_shape_constants_mirror_the_library():
    """_abi's keys per workgroup and scan step are the kernels' (the GPU test picks its sizes from them), and the scratch
    grows by a workgroup's histogram row exactly where one more workgroup is needed."""
    b, g = C.c_int(), C.c_int()
    assert rt.lib().rtc_ray_order_shape(C.byref(b), C.byref(g)) == 0
    assert (_abi.RAY_ORDER_KEYS_PER_GROUP, _abi.RAY_ORDER_SCAN_GROUPS) == (b.value, g.value) == (4096, 256)
    assert rt.lib().rtc_ray_order_shape(None, C.byref(g)) == RTC_EINVAL and b"rtc_ray_order_shape" in _msg()
    f = rt.ray_order_scratch_bytes
    assert f(b.value + 1) - f(b.value) >= 256 * 4 and f(2 * b.value + 1) - f(2 * b.value) >= 256 * 4
    assert f(b.value) - f(b.value - 63) == 0


def test_scratch_bytes():
    f = rt.ray_order_scratch_bytes
    ns = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 1 << 20, (1 << 20) + 1, 2073600, 0x7FFFFFFF]
    sizes = [f(n) for n in ns]
    assert all(s % 16 == 0 and s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    fine = [f(n) for n in range(0, 3 * 4096 + 2)]
    assert all(a <= b for a, b in zip(fine, fine[1:])) and all(s % 16 == 0 for s in fine)
    assert f(4097) > f(4096) and f(1 << 20) >= 3 * 4 * (1 << 20)  # three arrays of n words and the histograms


def test_async_refusals_come_before_any_device_call():
    f = rt.lib().rtc_ray_order_async
    for args, word in (((None, RAYS, 4, None, ORDER, KEYS, SCRATCH, BIG, None), b"null scene"),
                       ((FAKE, None, 4, None, ORDER, KEYS, SCRATCH, BIG, None), b"null"),
                       ((FAKE, RAYS, 4, None, None, KEYS, SCRATCH, BIG, None), b"null"),
                       ((FAKE, RAYS, 4, None, ORDER, None, None, BIG, None), b"null"),
                       ((FAKE, RAYS, 0x80000000, None, ORDER, None, SCRATCH, BIG, None), b"rays"),
                       ((FAKE, RAYS, 1 << 40, None, ORDER, None, SCRATCH, 1 << 62, None), b"rays"),
                       ((FAKE, RAYS, 4, None, ORDER, None, SCRATCH, rt.ray_order_scratch_bytes(4) - 1, None), b"scratch"),
                       ((FAKE, RAYS, 5000, None, ORDER, None, SCRATCH, rt.ray_order_scratch_bytes(4096), None), b"scratch"),
                       ((FAKE, RAYS, 4, None, ORDER, None, SCRATCH, 0, None), b"scratch"),
                       ((FAKE, RAYS, 4, None, ORDER, None, C.c_void_p(0x50008), BIG, None), b"aligned"),
                       ((FAKE, RAYS, 4, None, ORDER, None, C.c_void_p(0x50001), BIG, None), b"aligned")):
        assert f(*args) == RTC_EINVAL, args
        assert b"rtc_ray_order_async" in _msg() and word in _msg(), (args, _msg())


def test_no_rays_is_fine_and_enqueues_nothing():
    """n == 0 returns 0 before the handle is read; the refusals still come first."""
    f = rt.lib().rtc_ray_order_async
    assert f(FAKE, RAYS, 0, None, ORDER, KEYS, SCRATCH, rt.ray_order_scratch_bytes(0), None) == 0
    assert f(FAKE, RAYS, 0, None, ORDER, None, SCRATCH, BIG, None) == 0
    assert f(None, RAYS, 0, None, ORDER, None, SCRATCH, BIG, None) == RTC_EINVAL
    assert f(FAKE, RAYS, 0, None, ORDER, None, None, BIG, None) == RTC_EINVAL
    assert f(FAKE, RAYS, 0, None, ORDER, None, SCRATCH, rt.ray_order_scratch_bytes(0) - 16, None) == RTC_EINVAL
    assert f(FAKE, RAYS, 0, None, ORDER, None, C.c_void_p(0x50004), BIG, None) == RTC_EINVAL


def test_host_entry_refusals_and_enodev():
    L = rt.lib()
    rays, order = np.zeros(4, _abi.RAY_DT), np.full(4, 7, np.uint32)
    rp, op = rays.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p)
    f = L.rtc_ray_order
    assert f(None, rp, 4, None, op, None) == RTC_EINVAL and b"rtc_ray_order:" in _msg() and b"null scene" in _msg()
    assert f(FAKE, None, 4, None, op, None) == RTC_EINVAL and b"rtc_ray_order:" in _msg()
    assert f(FAKE, rp, 4, None, None, None) == RTC_EINVAL
    assert f(FAKE, rp, 1 << 31, None, op, None) == RTC_EINVAL and b"rays" in _msg()
    assert f(FAKE, rp, 0, None, op, None) == 0
    if rt.device_count() <= 0:  # (with a GPU the fake handle cannot be used: the GPU tests cover the entry)
        assert f(FAKE, rp, 4, None, op, None) == RTC_ENODEV
    assert (order == 7).all()


def test_scene_bounds_refusals():
    L = rt.lib()
    lo = (C.c_float * 3)()
    assert L.rtc_scene_bounds(None, lo, lo) == RTC_EINVAL and b"rtc_scene_bounds" in _msg()
    assert L.rtc_scene_bounds(FAKE, None, lo) == RTC_EINVAL and L.rtc_scene_bounds(FAKE, lo, None) == RTC_EINVAL


@pytest.mark.parametrize("name", ["rtc_gather_async", "rtc_scatter_async"])
def test_permutation_refusals(name):
    f = getattr(rt.lib(), name)
    dst, src = C.c_void_p(0x6000), C.c_void_p(0x7000)
    for args, word in (((None, src, ORDER, 4, 4, None), b"null"), ((dst, None, ORDER, 4, 4, None), b"null"),
                       ((dst, src, None, 4, 4, None), b"null"), ((dst, src, ORDER, 0x80000000, 4, None), b"elements"),
                       ((dst, src, ORDER, 4, 0, None), b"bytes"), ((dst, src, ORDER, 4, 2, None), b"bytes"),
                       ((dst, src, ORDER, 4, 3, None), b"bytes"), ((dst, src, ORDER, 4, 6, None), b"bytes"),
                       ((dst, src, ORDER, 4, 68, None), b"bytes"), ((dst, src, ORDER, 4, 128, None), b"bytes"),
                       ((dst, dst, ORDER, 4, 4, None), b"source"),
                       ((C.c_void_p(0x6002), src, ORDER, 4, 12, None), b"aligned"),
                       ((dst, C.c_void_p(0x7001), ORDER, 4, 24, None), b"aligned")):
        assert f(*args) == RTC_EINVAL, args
        assert name.encode() in _msg() and word in _msg(), (args, _msg())
    # nothing to move: fine for every element size the entries take, at any byte alignment for single bytes
    for eb in (1, 4, 12, 24, 64):
        assert f(dst, src, ORDER, 0, eb, None) == 0
    assert f(C.c_void_p(0x6001), C.c_void_p(0x7003), ORDER, 0, 1, None) == 0
    assert f(dst, src, ORDER, 0, 5, None) == RTC_EINVAL


def test_python_arguments_are_checked():
    ds = rt.DeviceScene.__new__(rt.DeviceScene)  # (no upload: the argument checks come first)
    ds._h = None
    with pytest.raises(ValueError):
        ds.ray_order(np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError):
        ds.ray_order(np.zeros((2, 6), np.float32), bounds=([0, 0, 0], [1, 1]))
    got = ds.ray_order(np.zeros((0, 6), np.float32))
    assert got.shape == (0,) and got.dtype == np.uint32
    order, keys = ds.ray_order(np.zeros(0, _abi.RAY_DT), keys=True)
    assert order.shape == keys.shape == (0,) and keys.dtype == np.uint32
    rays = np.zeros((3, 6), np.float32)
    for bad in ([0, 1], [0, 1, 3], [0, 1, -1], np.zeros((2, 3))):
        for call in (lambda o: ds.trace_rays(rays, order=o), lambda o: ds.occluded(rays, order=o),
                     lambda o: ds.trace_paths(rays, np.zeros(3, np.uint32), rt.default_scene(), 1, 1, order=o)):
            with pytest.raises(ValueError):
                call(bad)
    # no rays: nothing is ordered, whatever `order` says
    assert ds.trace_rays(np.zeros((0, 6), np.float32), order=True)["prim"].shape == (0,)
    assert ds.occluded(np.zeros((0, 6), np.float32), order=True).shape == (0,)
