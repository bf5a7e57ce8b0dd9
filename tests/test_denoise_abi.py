"""rtc_denoise_async / rtc_denoise_host at the C ABI (include/rtc.h): the symbols, the Python surface, the desc's
mirror, the shape constants, the scratch size, and every refusal -- all of which come before any device call, so they hold
without a GPU (fake addresses that are never dereferenced stand in for device buffers).  The values are
tests/test_denoise_reference.py's and tests/test_gpu_denoise.py's business."""
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
from raytracingc_amd._abi import RTC_EINVAL, RtcDenoiseDesc, RtcHitBuffers

ACC, SAMPLES, OUT, COLORS = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000), C.c_void_p(0x40001)
NORMAL, DEPTH, ALBEDO, SCRATCH = 0x50000, 0x60000, 0x70000, C.c_void_p(0x80000)
BIG = 1 << 60  # "enough scratch" for any size the refusals use


def _msg():
    return rt.lib().rtc_last_error()


def _desc(width=8, rows=4, iterations=3, flags=0, spp=8, squarings=2):
    return C.byref(RtcDenoiseDesc(width, rows, iterations, flags, spp, squarings, 1.0, 1.0, 0.01))


def _guides(normal=NORMAL, depth=DEPTH, albedo=ALBEDO):
    return C.byref(RtcHitBuffers(None, depth, normal, albedo))


def test_symbols_python_surface_and_desc_mirror():
    L = rt.lib()
    names = {"rtc_denoise_scratch_bytes", "rtc_denoise_shape", "rtc_denoise_async", "rtc_denoise_host"}
    assert all(hasattr(L, n) for n in names) and names <= set(_abi.EXPORTS)
    for f in ("denoise", "denoise_desc", "denoise_scratch_bytes", "denoise_async"):
        assert callable(getattr(rt, f)) and f in rt.__all__
    p = inspect.signature(rt.denoise).parameters
    assert list(p) == ["accum", "guides", "samples", "spp", "desc", "colors"]
    assert all(p[k].default is None for k in ("guides", "samples", "spp")) and p["colors"].default is False
    txt = open(os.path.join(REPO, "include", "rtc.h")).read()
    body = re.search(r"typedef struct RtcDenoiseDesc \{(.*?)\} RtcDenoiseDesc;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, f.strip()) for t, decl in re.findall(r"\b(float|int)\s+([^;]+);", body) for f in decl.split(",")]
    assert [f for _, f in fields] == [n for n, _ in RtcDenoiseDesc._fields_] and len(fields) == 9
    assert [{"float": C.c_float, "int": C.c_int}[t] for t, _ in fields] == [t for _, t in RtcDenoiseDesc._fields_]
    assert C.sizeof(RtcDenoiseDesc) == 36
    assert int(re.search(r"#define RTC_DN_DEMODULATE (\w+)", txt).group(1), 0) == _abi.RTC_DN_DEMODULATE == 1


def test_denoise_desc():
    d = rt.denoise_desc(48, 40, 4, 3, 0.5, 0.25, 0.01, True, 12)
    assert (d.width, d.rows, d.iterations, d.flags, d.spp, d.normalSquarings) == (48, 40, 4, 1, 12, 3)
    assert (d.depthScale, d.colorScale, d.albedoFloor) == (0.5, 0.25, np.float32(0.01))
    d = rt.denoise_desc(5, 6)
    assert (d.width, d.rows, d.iterations, d.flags) == (5, 6, 5, 0)


def test_shape_constants_mirror_the_library():
    w, h = C.c_int(), C.c_int()
    assert rt.lib().rtc_denoise_shape(C.byref(w), C.byref(h)) == 0
    assert (_abi.DENOISE_TILE_W, _abi.DENOISE_TILE_H) == (w.value, h.value)
    assert w.value >= 8 and h.value >= 8
    assert rt.lib().rtc_denoise_shape(None, C.byref(h)) == RTC_EINVAL and b"rtc_denoise_shape" in _msg()
    assert rt.lib().rtc_denoise_shape(C.byref(w), None) == RTC_EINVAL


def test_scratch_bytes():
    f = rt.denoise_scratch_bytes
    ns = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 1 << 20, (1 << 20) + 1, 2073600, 0x7FFFFFFF]
    for it in range(1, 7):
        sizes = [f(n, it) for n in ns]
        assert all(s % 16 == 0 for s in sizes) and all(s > 0 for s in sizes[1:])
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
        fine = [f(n, it) for n in range(0, 2100)]
        assert all(a <= b for a, b in zip(fine, fine[1:])) and all(s % 16 == 0 for s in fine)
    for n in ns:
        per = [f(n, it) for it in range(1, 7)]
        assert all(a <= b for a, b in zip(per, per[1:]))  # monotone in the iterations too
    # the guide entries and one colour image of 16 bytes a pixel each; a second colour image from two iterations on
    assert f(2073600, 1) == 2 * 16 * 2073600 and f(2073600, 5) == 3 * 16 * 2073600


def test_async_refusals_come_before_any_device_call():
    f = rt.lib().rtc_denoise_async
    need = rt.denoise_scratch_bytes(32, 3)
    # (argument order: accum, samples, guides, desc, out, colors, scratch, bytes, stream)
    for args, word in (((None, SAMPLES, _guides(), _desc(), OUT, COLORS, SCRATCH, BIG, None), b"null"),
                       ((ACC, SAMPLES, _guides(), None, OUT, COLORS, SCRATCH, BIG, None), b"null"),
                       ((ACC, SAMPLES, _guides(), _desc(), None, COLORS, SCRATCH, BIG, None), b"null"),
                       ((ACC, SAMPLES, _guides(), _desc(width=0), OUT, COLORS, SCRATCH, BIG, None), b"image"),
                       ((ACC, SAMPLES, _guides(), _desc(width=-3), OUT, COLORS, SCRATCH, BIG, None), b"image"),
                       ((ACC, SAMPLES, _guides(), _desc(rows=0), OUT, COLORS, SCRATCH, BIG, None), b"image"),
                       ((ACC, SAMPLES, _guides(), _desc(rows=-1), OUT, COLORS, SCRATCH, BIG, None), b"image"),
                       ((ACC, SAMPLES, _guides(), _desc(width=1 << 16, rows=1 << 15), OUT, COLORS, SCRATCH, BIG, None),
                        b"pixels"),
                       ((ACC, SAMPLES, _guides(), _desc(width=0x7fffffff, rows=2), OUT, COLORS, SCRATCH, BIG, None),
                        b"pixels"),
                       ((ACC, SAMPLES, _guides(), _desc(iterations=0), OUT, COLORS, SCRATCH, BIG, None), b"iterations"),
                       ((ACC, SAMPLES, _guides(), _desc(iterations=7), OUT, COLORS, SCRATCH, BIG, None), b"iterations"),
                       ((ACC, SAMPLES, _guides(), _desc(squarings=-1), OUT, COLORS, SCRATCH, BIG, None), b"normalSquarings"),
                       ((ACC, SAMPLES, _guides(), _desc(squarings=9), OUT, COLORS, SCRATCH, BIG, None), b"normalSquarings"),
                       ((ACC, SAMPLES, _guides(), _desc(flags=2), OUT, COLORS, SCRATCH, BIG, None), b"flag"),
                       ((ACC, SAMPLES, _guides(), _desc(flags=0x11), OUT, COLORS, SCRATCH, BIG, None), b"flag"),
                       ((ACC, SAMPLES, _guides(albedo=None), _desc(flags=1), OUT, COLORS, SCRATCH, BIG, None), b"albedo"),
                       ((ACC, SAMPLES, None, _desc(flags=1), OUT, COLORS, SCRATCH, BIG, None), b"albedo"),
                       ((ACC, SAMPLES, _guides(), _desc(spp=0), OUT, COLORS, SCRATCH, BIG, None), b"spp"),
                       ((ACC, SAMPLES, _guides(), _desc(spp=-2), OUT, COLORS, SCRATCH, BIG, None), b"spp"),
                       ((ACC, SAMPLES, _guides(), _desc(), ACC, COLORS, SCRATCH, BIG, None), b"is the accumulator"),
                       ((ACC, SAMPLES, _guides(), _desc(), OUT, COLORS, None, BIG, None), b"null scratch"),
                       ((ACC, SAMPLES, _guides(), _desc(), OUT, COLORS, C.c_void_p(0x80008), BIG, None), b"aligned"),
                       ((ACC, SAMPLES, _guides(), _desc(), OUT, COLORS, C.c_void_p(0x80001), BIG, None), b"aligned"),
                       ((ACC, SAMPLES, _guides(), _desc(), OUT, COLORS, SCRATCH, need - 1, None), b"scratch"),
                       ((ACC, SAMPLES, _guides(), _desc(), OUT, COLORS, SCRATCH, 0, None), b"scratch"),
                       # one iteration's scratch does not serve three
                       ((ACC, SAMPLES, _guides(), _desc(), OUT, COLORS, SCRATCH, rt.denoise_scratch_bytes(32, 1), None),
                        b"scratch")):
        assert f(*args) == RTC_EINVAL, args
        assert b"rtc_denoise_async" in _msg() and word in _msg(), (args, _msg())
    # spp counts only with sample counts: without them the next refusal in line is reached
    assert f(ACC, None, _guides(), _desc(spp=0), OUT, COLORS, None, BIG, None) == RTC_EINVAL and b"null scratch" in _msg()
    # the largest image that is allowed gets as far as the scratch
    assert f(ACC, None, None, _desc(width=0x7fffffff, rows=1), OUT, None, None, BIG, None) == RTC_EINVAL
    assert b"null scratch" in _msg()


def test_host_refusals():
    f = rt.lib().rtc_denoise_host
    acc, out = np.zeros((4, 8, 3), np.float32), np.full((4, 8, 3), 7, np.float32)
    samples, colors = np.full((4, 8), 8, np.int32), np.full((4, 8, 3), 9, np.uint8)
    normal, depth, albedo = np.zeros((4, 8, 3), np.float32), np.zeros((4, 8), np.float32), np.ones((4, 8, 3), np.float32)
    a, s, o, c = (x.ctypes.data_as(C.c_void_p) for x in (acc, samples, out, colors))

    def g(with_albedo=True):
        return C.byref(RtcHitBuffers(None, depth.ctypes.data, normal.ctypes.data, albedo.ctypes.data if with_albedo else None))

    for args, word in (((None, s, g(), _desc(), o, c), b"null"), ((a, s, g(), None, o, c), b"null"),
                       ((a, s, g(), _desc(), None, c), b"null"),
                       ((a, s, g(), _desc(width=0), o, c), b"image"), ((a, s, g(), _desc(rows=-1), o, c), b"image"),
                       ((a, s, g(), _desc(width=1 << 16, rows=1 << 15), o, c), b"pixels"),
                       ((a, s, g(), _desc(iterations=0), o, c), b"iterations"),
                       ((a, s, g(), _desc(iterations=7), o, c), b"iterations"),
                       ((a, s, g(), _desc(squarings=-1), o, c), b"normalSquarings"),
                       ((a, s, g(), _desc(squarings=9), o, c), b"normalSquarings"),
                       ((a, s, g(), _desc(flags=4), o, c), b"flag"),
                       ((a, s, g(False), _desc(flags=1), o, c), b"albedo"), ((a, s, None, _desc(flags=1), o, c), b"albedo"),
                       ((a, s, g(), _desc(spp=0), o, c), b"spp"),
                       ((a, s, g(), _desc(), a, c), b"is the accumulator")):
        assert f(*args) == RTC_EINVAL, args
        assert b"rtc_denoise_host" in _msg() and word in _msg(), (args, _msg())
    assert (out == 7).all() and (colors == 9).all()  # a refused call writes nothing
    # what is allowed: no guides, no samples (spp is then ignored), no colors
    assert f(a, None, None, _desc(spp=0), o, None) == 0 and (out == 0).all() and (colors == 9).all()
    assert f(a, s, g(), _desc(flags=1), o, c) == 0 and (colors == 0).all()


def test_python_arguments_are_checked():
    acc = np.zeros((4, 8, 3), np.float32)
    with pytest.raises(ValueError):
        rt.denoise(np.zeros((4, 8), np.float32))
    with pytest.raises(ValueError):
        rt.denoise(acc, desc=rt.denoise_desc(4, 8))
    with pytest.raises(ValueError):
        rt.denoise(acc, samples=np.ones((4, 8), np.int32))
    with pytest.raises(ValueError):
        rt.denoise(acc, spp=8)
    with pytest.raises(ValueError):
        rt.denoise(acc, samples=np.ones((4, 7), np.int32), spp=8)
    with pytest.raises(ValueError):
        rt.denoise(acc, guides={"normal": np.zeros((4, 8), np.float32)})
    with pytest.raises(rt.RtcError):
        rt.denoise(acc, desc=rt.denoise_desc(8, 4, demodulate=True))
    out = rt.denoise(acc, guides={"prim": np.zeros((4, 8), np.int32), "albedo": None})  # (prim is ignored)
    assert out.shape == acc.shape and out.dtype == np.float32
    out, colors = rt.denoise(acc + 1, colors=True)
    assert (colors == 255).all() and colors.shape == acc.shape
