"""rtc_select_pixels_async / rtc_select_pixels_host / rtc_resolve_async / rtc_resolve_host at the C ABI (include/rtc.h;
DESIGN 3.20): the symbols, the Python surface, the shape constants, the scratch size, and every refusal -- all of which
come before any device call, so they hold without a GPU (fake addresses that are never dereferenced stand in for device
buffers).  The values are tests/test_select_reference.py's and tests/test_gpu_select.py's business."""
from __future__ import annotations

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

import raytracingc_amd as rt
from raytracingc_amd import _abi
from raytracingc_amd._abi import RTC_EINVAL, RtcSelectDesc

ACC, PREV = C.c_void_p(0x10000), C.c_void_p(0x20000)  # "device" buffers that must never be dereferenced
IN, OUT, COUNT, SAMPLES = C.c_void_p(0x30000), C.c_void_p(0x40000), C.c_void_p(0x50000), C.c_void_p(0x60000)
SCRATCH, COLORS = C.c_void_p(0x70000), C.c_void_p(0x80001)
BIG = 1 << 40  # "enough scratch" for any size the refusals use
TOO_MANY = 0x80000000


def _msg():
    return rt.lib().rtc_last_error()


def _sel(done=8):
    return C.byref(RtcSelectDesc(1.0, 2.0, 1.0, 0.01, 0.1, done))


def test_symbols_python_surface_and_desc_mirror():
    L = rt.lib()
    names = {"rtc_select_scratch_bytes", "rtc_select_shape", "rtc_select_pixels_async", "rtc_select_pixels_host",
             "rtc_resolve_async", "rtc_resolve_host"}
    assert all(hasattr(L, n) for n in names) and names <= set(_abi.EXPORTS)
    for f in ("select_pixels", "select_scratch_bytes", "resolve", "select_desc", "select_pixels_async", "resolve_async"):
        assert callable(getattr(rt, f)) and f in rt.__all__
    p = inspect.signature(rt.select_pixels).parameters
    assert list(p) == ["accum", "prev", "sel", "pixels", "capacity", "samples"]
    assert all(p[k].default is None for k in ("pixels", "capacity", "samples"))
    p = inspect.signature(rt.DeviceScene.render_adaptive_device).parameters
    assert list(p) == ["self", "scene", "cam", "cfg", "passes", "threshold", "floor", "capacity", "flags"]
    assert p["flags"].default == rt.RTC_F_WAVE_PER_RAY
    # the ctypes struct has the header's fields in the header's order
    txt = open(os.path.join(REPO, "include", "rtc.h")).read()
    body = re.search(r"typedef struct RtcSelectDesc \{(.*?)\} RtcSelectDesc;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, f.strip()) for t, decl in re.findall(r"\b(float|int)\s+([^;]+);", body) for f in decl.split(",")]
    assert [f for _, f in fields] == [n for n, _ in RtcSelectDesc._fields_] and len(fields) == 6
    assert [{"float": C.c_float, "int": C.c_int}[t] for t, _ in fields] == [t for _, t in RtcSelectDesc._fields_]
    assert C.sizeof(RtcSelectDesc) == 24


def test_select_desc_weights():
    """rt.select_desc: the issue's weights in double, rounded once; samplesDone = done."""
    d = rt.select_desc(1024, 64, 128, 0.25, 0.5)
    assert (d.wAccum, d.wPrev, d.wLevel, d.floor, d.threshold, d.samplesDone) == (16.0, 32.0, 8.0, 0.5, 0.25, 128)
    d = rt.select_desc(12, 6, 8, 0.1, 0.02)
    F = np.float32
    assert d.wAccum == 6.0 and d.wPrev == 8.0 and d.wLevel == 1.5 and d.threshold == F(0.1) and d.floor == F(0.02)
    d = rt.select_desc(100, 3, 10, 1, 1)
    assert d.wAccum == F(100 / 7) and d.wPrev == F(100 / 7 + 100 / 3) and d.wLevel == 10.0
    for bad in ((12, 0, 4), (12, 4, 4), (12, 5, 4), (0, 1, 2)):
        with pytest.raises(ValueError):
            rt.select_desc(*bad, 0.1, 0.1)


def test_shape_constants_mirror_the_library():
    t, g = C.c_int(), C.c_int()
    assert rt.lib().rtc_select_shape(C.byref(t), C.byref(g)) == 0
    assert (_abi.SELECT_ENTRIES_PER_GROUP, _abi.SELECT_SCAN_GROUPS) == (t.value, g.value)
    assert t.value % 64 == 0 and t.value >= 256 and g.value >= 64
    assert rt.lib().rtc_select_shape(None, C.byref(g)) == RTC_EINVAL and b"rtc_select_shape" in _msg()
    assert rt.lib().rtc_select_shape(C.byref(t), None) == RTC_EINVAL
    f = rt.select_scratch_bytes
    assert f(t.value + 1) > f(t.value - 63) and f(g.value * t.value + 1) > f(g.value * t.value)
    assert _abi.SELECT_SENTINEL == 0xFFFFFFFF


def test_scratch_bytes():
    f = rt.select_scratch_bytes
    t = _abi.SELECT_ENTRIES_PER_GROUP
    ns = [0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1, 1 << 20, (1 << 20) + 1, 2073600, 0x7FFFFFFF]
    sizes = [f(n) for n in ns]
    assert all(s % 16 == 0 and s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    fine = [f(n) for n in range(0, 3 * t + 2)]
    assert all(a <= b for a, b in zip(fine, fine[1:])) and all(s % 16 == 0 for s in fine)
    assert f(2073600) >= 2073600 // 8 and f(2073600) < 2073600  # a bit per entry and a count per tile: well below the list


def test_async_refusals_come_before_any_device_call():
    f = rt.lib().rtc_select_pixels_async
    ok = f  # (argument order: accum, prev, pixels, in, nIn, sel, out, capacity, count, samples, scratch, bytes, stream)
    for args, word in (((None, PREV, 100, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"null"),
                       ((ACC, None, 100, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"null"),
                       ((ACC, PREV, 100, IN, 4, None, OUT, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"null"),
                       ((ACC, PREV, TOO_MANY, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"pixels"),
                       ((ACC, PREV, 100, IN, TOO_MANY, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"entries"),
                       ((ACC, PREV, 100, IN, 4, _sel(), OUT, TOO_MANY, COUNT, SAMPLES, SCRATCH, BIG, None), b"capacity"),
                       ((ACC, PREV, 1 << 40, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, 1 << 62, None), b"pixels"),
                       ((ACC, PREV, 100, None, 4, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"no input list"),
                       ((ACC, PREV, 100, IN, 4, _sel(), None, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"no output list"),
                       ((ACC, PREV, 100, IN, 4, _sel(), None, 0, None, None, SCRATCH, BIG, None), b"no output"),
                       ((ACC, PREV, 100, IN, 4, _sel(), IN, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"is the input list"),
                       ((ACC, PREV, 100, IN, 4, _sel(-1), OUT, 4, COUNT, SAMPLES, SCRATCH, BIG, None), b"samplesDone"),
                       ((ACC, PREV, 100, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, None, BIG, None), b"null scratch"),
                       ((ACC, PREV, 100, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, C.c_void_p(0x70008), BIG, None), b"aligned"),
                       ((ACC, PREV, 100, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, C.c_void_p(0x70001), BIG, None), b"aligned"),
                       ((ACC, PREV, 100, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, rt.select_scratch_bytes(4) - 1, None),
                        b"scratch"),
                       ((ACC, PREV, 100, IN, 4, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, 0, None), b"scratch"),
                       # without a list the sequence is every pixel: the scratch is sized by the pixel count
                       ((ACC, PREV, 5000, None, 0, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, rt.select_scratch_bytes(2048), None),
                        b"scratch"),
                       ((ACC, PREV, 100, IN, 5000, _sel(), OUT, 4, COUNT, SAMPLES, SCRATCH, rt.select_scratch_bytes(100), None),
                        b"scratch")):
        assert ok(*args) == RTC_EINVAL, args
        assert b"rtc_select_pixels_async" in _msg() and word in _msg(), (args, _msg())
    # a negative samplesDone is refused only where it would be stamped
    assert f(ACC, PREV, 100, IN, 4, _sel(-1), OUT, 4, COUNT, None, None, BIG, None) == RTC_EINVAL and b"null scratch" in _msg()


def test_host_refusals():
    f = rt.lib().rtc_select_pixels_host
    acc, prev = np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32)
    lst, out, samples = np.arange(4, dtype=np.uint32), np.full(4, 7, np.uint32), np.full(8, -3, np.int32)
    count = C.c_ulonglong(99)
    a, p, i, o, s = (x.ctypes.data_as(C.c_void_p) for x in (acc, prev, lst, out, samples))
    c = C.cast(C.pointer(count), C.c_void_p)
    for args, word in (((None, p, 8, i, 4, _sel(), o, 4, c, s), b"null"), ((a, None, 8, i, 4, _sel(), o, 4, c, s), b"null"),
                       ((a, p, 8, i, 4, None, o, 4, c, s), b"null"),
                       ((a, p, TOO_MANY, i, 4, _sel(), o, 4, c, s), b"pixels"),
                       ((a, p, 8, i, TOO_MANY, _sel(), o, 4, c, s), b"entries"),
                       ((a, p, 8, i, 4, _sel(), o, TOO_MANY, c, s), b"capacity"),
                       ((a, p, 8, None, 4, _sel(), o, 4, c, s), b"no input list"),
                       ((a, p, 8, i, 4, _sel(), None, 4, c, s), b"no output list"),
                       ((a, p, 8, i, 4, _sel(), None, 0, None, None), b"no output"),
                       ((a, p, 8, i, 4, _sel(), i, 4, c, s), b"is the input list"),
                       ((a, p, 8, i, 4, _sel(-1), o, 4, c, s), b"samplesDone")):
        assert f(*args) == RTC_EINVAL, args
        assert b"rtc_select_pixels_host" in _msg() and word in _msg(), (args, _msg())
    assert (out == 7).all() and (samples == -3).all() and count.value == 99  # a refused call writes nothing
    # what is allowed: no list at all (count and samples only), a negative samplesDone that is not stamped
    assert f(a, p, 8, i, 4, _sel(), None, 0, c, None) == 0 and count.value == 0
    assert f(a, p, 8, i, 4, _sel(-1), o, 4, None, None) == 0 and (out == 0xFFFFFFFF).all()
    assert f(a, p, 8, None, 0, _sel(5), None, 0, None, s) == 0 and (samples == 5).all()


@pytest.mark.parametrize("name", ["rtc_resolve_async", "rtc_resolve_host"])
def test_resolve_refusals(name):
    f = getattr(rt.lib(), name)
    tail = (None,) if name.endswith("async") else ()
    for args, word in (((None, SAMPLES, 4, 8, COLORS), b"null"), ((ACC, None, 4, 8, COLORS), b"null"),
                       ((ACC, SAMPLES, 4, 8, None), b"null"), ((ACC, SAMPLES, 4, 0, COLORS), b"spp"),
                       ((ACC, SAMPLES, 4, -1, COLORS), b"spp"), ((ACC, SAMPLES, TOO_MANY, 8, COLORS), b"pixels"),
                       ((ACC, SAMPLES, 1 << 40, 8, COLORS), b"pixels"), ((None, SAMPLES, 0, 8, COLORS), b"null"),
                       ((ACC, SAMPLES, 0, 0, COLORS), b"spp")):
        assert f(*args, *tail) == RTC_EINVAL, args
        assert name.encode() in _msg() and word in _msg(), (args, _msg())
    assert f(ACC, SAMPLES, 0, 8, COLORS, *tail) == 0  # no pixels: nothing is read, written or enqueued


def test_python_arguments_are_checked():
    acc = np.zeros((4, 3), np.float32)
    d = rt.select_desc(8, 2, 4, 0.1, 0.1)
    with pytest.raises(ValueError):
        rt.select_pixels(np.zeros(7, np.float32), np.zeros(7, np.float32), d)
    with pytest.raises(ValueError):
        rt.select_pixels(acc, np.zeros((5, 3), np.float32), d)
    with pytest.raises(ValueError):
        rt.select_pixels(acc, acc, d, samples=np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        rt.select_pixels(acc, acc, d, pixels=[0, -1])
    with pytest.raises(ValueError):
        rt.resolve(acc, np.zeros(5, np.int32), 8)
    with pytest.raises(rt.RtcError):
        rt.resolve(acc, np.zeros(4, np.int32), 0)
    out, count = rt.select_pixels(acc, acc, d, pixels=[])
    assert out.shape == (0,) and count == 0
    out, count = rt.select_pixels(acc, acc, d, pixels=[], capacity=3)
    assert (out == 0xFFFFFFFF).all() and len(out) == 3 and count == 0
    ds = rt.DeviceScene.__new__(rt.DeviceScene)  # (no upload: the argument checks come first)
    ds._h = None
    cfg = rt.RenderConfig(8, 8, 8, 2, True)
    for passes, cap in (([8], 4), ([4, 0], 4), ([4, 5], 4), ([4, 4], 0), ([4, 4], 1 << 31)):
        with pytest.raises(ValueError):
            ds.render_adaptive_device(rt.default_scene(), rt.camera_basis(), cfg, passes, 0.1, 0.1, cap)
