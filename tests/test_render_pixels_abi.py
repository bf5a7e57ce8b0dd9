"""rtc_render_pixels_async / rtc_render_pixels at the C ABI (include/rtc.h): the symbols, the Python surface
and the refusals that come before any device call and before the scene handle is read, so they hold without a GPU (a fake
handle that is never dereferenced stands in for a scene).  The values are tests/test_gpu_render_pixels.py's business.
Reference seam: main.c:88-100 for the listed pixels alone."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import raytracingc_amd as rt
from raytracingc_amd import _abi
from raytracingc_amd._abi import RTC_EINVAL, RTC_ENODEV, RtcRenderDesc, RtcSampleRange

FAKE = C.c_void_p(0x10)      # a scene handle that must never be dereferenced
PIXELS = C.c_void_p(0x2000)  # nor these "device" buffers
ACCUM = C.c_void_p(0x3000)
STATE = C.c_void_p(0x4000)
COLORS = C.c_void_p(0x5000)
NO_CULL, WAVE = rt.RTC_F_NO_CLUSTER_CULL, rt.RTC_F_WAVE_PER_RAY
SCENE, CAM = rt.default_scene(), rt.camera_basis()


def _desc(w=64, h=40, spp=12, mb=4, tonly=1, row_start=0, stride=1, flags=0, band=0):
    return RtcRenderDesc(w, h, spp, mb, tonly, row_start, stride, flags, band)


def _msg():
    return rt.lib().rtc_last_error()


def _async(s=FAKE, scene=SCENE, cam=CAM, d=None, rg=(5, 7), pixels=PIXELS, n=4, flags=0, colors=COLORS, accum=ACCUM,
           rng=STATE, seg=None, null_desc=False):
    d = _desc() if d is None else d
    return rt.lib().rtc_render_pixels_async(s, C.byref(scene) if scene is not None else None,
                                            C.byref(cam) if cam is not None else None, None if null_desc else C.byref(d),
                                            C.byref(RtcSampleRange(*rg)) if rg is not None else None, pixels, n, flags,
                                            colors, accum, rng, seg, None)


# every refusal of the contract's list, as keyword arguments of _async / _host, with a word of the message
REFUSALS = {
    "null scene handle": (dict(s=None), b"null scene"),
    "null Scene": (dict(scene=None), b"null"),
    "null camera": (dict(cam=None), b"null"),
    "null desc": (dict(null_desc=True), b"null"),
    "null range": (dict(rg=None), b"null"),
    "null list": (dict(pixels=None), b"null"),
    "null accumulator": (dict(accum=None), b"null"),
    "null state buffer": (dict(rng=None), b"null"),
    "n = 2^31": (dict(n=0x80000000), b"at most"),
    "n = 2^40": (dict(n=1 << 40), b"at most"),
    "width 0": (dict(d=_desc(w=0)), b"geometry"),
    "height -1": (dict(d=_desc(h=-1)), b"geometry"),
    "row stride 0": (dict(d=_desc(stride=0)), b"geometry"),
    "row start -1": (dict(d=_desc(row_start=-1)), b"geometry"),
    "band 128": (dict(d=_desc(band=128)), b"geometry"),
    "band 3": (dict(d=_desc(band=3)), b"geometry"),
    "frame too large": (dict(d=_desc(w=1 << 15, h=1 << 15)), b"too large"),
    "spp 0": (dict(d=_desc(spp=0), rg=(0, 1)), b"spp"),
    "spp -3": (dict(d=_desc(spp=-3), rg=(0, 1)), b"spp"),
    "first -1": (dict(rg=(-1, 1)), b"samples"),
    "count 0": (dict(rg=(5, 0)), b"samples"),
    "count -2": (dict(rg=(5, -2)), b"samples"),
    "range past spp": (dict(rg=(6, 7)), b"samples"),
    "range past spp, huge count": (dict(rg=(2, 0x7fffffff)), b"samples"),
    "tile-cull flag": (dict(flags=rt.RTC_F_NO_TILE_CULL), b"flags"),
    "overlap as the entry's flag": (dict(flags=rt.RTC_F_OVERLAP), b"flags"),
    "debug as the entry's flag": (dict(flags=rt.RTC_F_DEBUG_BOUNCES), b"flags"),
    "cull flag and another": (dict(flags=NO_CULL | rt.RTC_F_HOIST_PRIMARY), b"flags"),
    "unknown flag": (dict(flags=0x40000000), b"flags"),
    "desc: debug bounces": (dict(d=_desc(flags=rt.RTC_F_DEBUG_BOUNCES)), b"RTC_F_DEBUG_BOUNCES"),
    "desc: overlap": (dict(d=_desc(flags=rt.RTC_F_OVERLAP)), b"RTC_F_OVERLAP"),
    "desc: coop4": (dict(d=_desc(flags=_abi.RTC_F_COOP4)), b"removed"),
    "desc: coop8": (dict(d=_desc(flags=_abi.RTC_F_COOP8)), b"removed"),
    "desc: pipe": (dict(d=_desc(flags=_abi.RTC_F_PIPE)), b"removed"),
    "desc: spec": (dict(d=_desc(flags=_abi.RTC_F_SPEC)), b"removed"),
}


def test_symbols_and_python_surface():
    L = rt.lib()
    names = {"rtc_render_pixels_async", "rtc_render_pixels", "rtc_plan_sim_render_pixels"}
    assert all(hasattr(L, n) for n in names) and names <= set(_abi.EXPORTS)
    for m in ("render_pixels_async", "render_pixels", "render_adaptive"):
        assert hasattr(rt.DeviceScene, m)


def test_abi_matches_the_header():
    """The parameter lists include/rtc.h declares for the three entries, against the ctypes declarations."""
    import os

    text = open(os.path.join(os.path.dirname(os.path.abspath(rt.__file__)), "..", "include", "rtc.h")).read()
    kinds = {"vp": C.c_void_p, "sz": C.c_size_t, "ip": C.c_int, "ull": C.c_ulonglong}

    def kind(param):
        p = re.sub(r"/\*.*?\*/", "", param).strip()
        if "*" in p or "[" in p:
            for ty, ct in (("Scene", _abi.Scene), ("RtcCamera", _abi.RtcCamera), ("RtcRenderDesc", RtcRenderDesc),
                           ("RtcSampleRange", RtcSampleRange)):
                if re.match(rf"const {ty} \*", p):
                    return C.POINTER(ct)
            return kinds["vp"]
        return {"size_t": kinds["sz"], "int": kinds["ip"], "unsigned long long": kinds["ull"]}[p.rsplit(" ", 1)[0]]

    for name in ("rtc_render_pixels_async", "rtc_render_pixels", "rtc_plan_sim_render_pixels"):
        m = re.search(rf"\nint {name}\((.*?)\);", text, re.S)
        assert m, name
        params = [q for q in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert [kind(q) for q in params] == list(getattr(rt.lib(), name).argtypes), name


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_async_refusals_come_before_any_device_call(what):
    kw, word = REFUSALS[what]
    assert _async(**kw) == RTC_EINVAL
    assert b"rtc_render_pixels_async" in _msg() and word in _msg()


def test_accepted_calls_and_nothing_to_do():
    """n == 0 returns 0 before the handle is read, for every accepted range, flag and desc; so does a launch that selects
    no row; the refusals still come first."""
    for kw in (dict(), dict(flags=NO_CULL), dict(flags=WAVE), dict(flags=NO_CULL | WAVE), dict(rg=(0, 12)), dict(rg=(11, 1)),
               dict(rg=(0, 1)), dict(colors=None), dict(seg=C.c_void_p(0x6000)), dict(d=_desc(mb=0)), dict(d=_desc(mb=-5)),
               dict(d=_desc(spp=0x7fffffff), rg=(0x7ffffffe, 1)), dict(d=_desc(row_start=1, stride=3)),
               dict(d=_desc(stride=2, band=8)),
               # the frame's own route flags are ignored: the desc of the whole passes is accepted as it is
               dict(d=_desc(flags=rt.RTC_F_HOIST_PRIMARY | rt.RTC_F_NO_TILE_CULL | rt.RTC_F_NO_REORDER | rt.RTC_F_NO_COOP |
                            NO_CULL | rt.RTC_F_CHAIN_INLINE | rt.RTC_F_SPLIT_SPHERES | rt.RTC_F_NO_DRAW_CACHE))):
        assert _async(n=0, **kw) == 0, kw
    assert _async(n=4, d=_desc(h=2, row_start=2, stride=3)) == 0  # rows_selected == 0: nothing enqueued
    assert _async(n=0, d=_desc(flags=rt.RTC_F_OVERLAP)) == RTC_EINVAL
    assert _async(n=0, flags=rt.RTC_F_HOIST_PRIMARY) == RTC_EINVAL
    assert _async(n=0, s=None) == RTC_EINVAL


def _host(s=FAKE, scene=SCENE, cam=CAM, d=None, rg=(5, 7), pixels=True, n=4, flags=0, colors=True, accum=True, rng=True,
          null_desc=False):
    d = _desc() if d is None else d
    npx = 64 * 40
    a = {"pixels": np.zeros(4, np.uint32), "colors": np.zeros((npx, 3), np.uint8), "accum": np.zeros((npx, 3), np.float32),
         "rng": np.zeros(npx, np.uint32)}
    p = lambda k, on: a[k].ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    return rt.lib().rtc_render_pixels(s, C.byref(scene) if scene is not None else None,
                                      C.byref(cam) if cam is not None else None, None if null_desc else C.byref(d),
                                      C.byref(RtcSampleRange(*rg)) if rg is not None else None, p("pixels", pixels), n, flags,
                                      p("colors", colors), p("accum", accum), p("rng", rng), None)


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_host_entry_has_the_same_refusals(what):
    kw, word = dict(REFUSALS[what][0]), REFUSALS[what][1]
    for k in ("pixels", "accum", "rng"):
        if k in kw:
            kw[k] = False
    assert _host(**kw) == RTC_EINVAL
    assert b"rtc_render_pixels:" in _msg() and word in _msg()


def test_host_entry_nothing_to_do_and_no_gpu():
    """n == 0 is fine; without a device the host entry returns RTC_ENODEV before it reads the handle (with one, the fake
    handle cannot be used: the GPU tests cover the entry)."""
    assert _host(n=0) == 0
    assert _host(colors=False, n=0) == 0
    if rt.device_count() > 0:
        return  # (tests/test_gpu_render_pixels.py runs the host entry on a real scene)
    assert _host() == RTC_ENODEV
    assert _host(rg=(6, 7)) == RTC_EINVAL  # the refusals come first


def test_python_arguments_are_checked():
    ds = rt.DeviceScene.__new__(rt.DeviceScene)  # (no upload: the argument checks come first)
    ds._h = None
    cfg = rt.RenderConfig(8, 4, 12, 4, True)
    acc, rng, col = np.zeros((4, 8, 3), np.float32), np.zeros((4, 8), np.uint32), np.zeros((4, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        ds.render_pixels(SCENE, CAM, cfg, 0, 12, [0, 1], acc[:3], rng)
    with pytest.raises(ValueError):
        ds.render_pixels(SCENE, CAM, cfg, 0, 12, [0, 1], acc, rng[:3])
    with pytest.raises(ValueError):
        ds.render_pixels(SCENE, CAM, cfg, 0, 12, [0, 1], acc, rng, colors=col[:3])
    with pytest.raises(ValueError):
        ds.render_pixels(SCENE, CAM, cfg, 0, 12, [0, -1], acc, rng)
    with pytest.raises(ValueError):
        ds.render_pixels(SCENE, CAM, cfg, 0, 12, [0.5], acc, rng)
    got = ds.render_pixels(SCENE, CAM, cfg, 0, 12, np.zeros(0, np.uint32), acc, rng, colors=col, segments=True)
    assert set(got) == {"accum", "rng", "colors", "segments"} and got["segments"] == 0
    assert got["accum"] is not acc and np.array_equal(got["accum"], acc) and got["rng"].dtype == np.uint32


def test_adaptive_selection_is_validated():
    """What render_adaptive accepts from its callback (rt.adaptive_selection, no GPU): a subset of the previous pass's
    pixels, all at samples == done, none twice; anything else raises ValueError."""
    samples = np.full((4, 8), 5, np.int32)
    samples[0, :4] = 9  # the previous pass took pixels 0 .. 3 on to 9
    ok = rt.adaptive_selection([3, 0, 2], samples, 9)
    assert ok.dtype == np.uint32 and ok.tolist() == [3, 0, 2]
    assert rt.adaptive_selection(np.array([1], np.int64), samples, 9).tolist() == [1]
    assert len(rt.adaptive_selection([], samples, 9)) == 0 and len(rt.adaptive_selection(np.zeros(0), samples, 9)) == 0
    for bad in ([0, 4], [7], [0, 0], [32], [-1], [1 << 40], [0.5], [[0, 31]]):
        with pytest.raises(ValueError):
            rt.adaptive_selection(bad, samples, 9)
    with pytest.raises(ValueError):
        rt.adaptive_selection([0], samples, 5)  # a pixel that went past `done`: not of the previous pass
