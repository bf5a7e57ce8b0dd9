"""rtc_render_first_hit_async at the C ABI (include/rtc.h): the symbol, the layout of RtcHitBuffers and the
refusals that come before any device call, so they hold without a GPU.  The values are tests/test_gpu_first_hit.py's
business.  Reference seam: calculateRayCollision (raytracing.c:216-240) on the primary ray of main.c:88-94."""
from __future__ import annotations

import ctypes as C
import os
import re

from conftest import REPO

import raytracingc_amd as rt
from raytracingc_amd import _abi


def test_symbol_and_python_surface():
    L = rt.lib()
    assert hasattr(L, "rtc_render_first_hit_async") and hasattr(L, "rtc_plan_sim_set_first_hit")
    assert {"rtc_render_first_hit_async", "rtc_plan_sim_set_first_hit"} <= set(_abi.EXPORTS)
    assert hasattr(rt.DeviceScene, "render_first_hit_async") and hasattr(rt.DeviceScene, "first_hit")


def test_hit_buffers_layout_matches_header():
    """Four pointers, 32 bytes, in the header's order: prim, depth, normal, albedo."""
    assert C.sizeof(_abi.RtcHitBuffers) == 32
    txt = open(os.path.join(REPO, "include", "rtc.h")).read()
    body = re.search(r"typedef struct RtcHitBuffers \{(.*?)\} RtcHitBuffers;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert fields == [n for n, _ in _abi.RtcHitBuffers._fields_] == ["prim", "depth", "normal", "albedo"]
    assert [getattr(_abi.RtcHitBuffers, n).offset for n in fields] == [0, 8, 16, 24]


def test_null_scene_and_null_out_are_refused_with_a_message():
    L = rt.lib()
    cam = rt.camera_basis()
    d = _abi.RtcRenderDesc(16, 16, 0, 0, 1, 0, 1, 0, 0)
    out = _abi.RtcHitBuffers(C.c_void_p(0x1000), None, None, None)
    assert L.rtc_render_first_hit_async(None, C.byref(cam), C.byref(d), C.byref(out), None) == _abi.RTC_EINVAL
    msg = L.rtc_last_error()
    assert b"rtc_render_first_hit_async" in msg and b"null scene" in msg
    # a scene handle that is never dereferenced: the null `out` is refused first
    fake = C.c_void_p(0x10)
    assert L.rtc_render_first_hit_async(fake, C.byref(cam), C.byref(d), None, None) == _abi.RTC_EINVAL
    msg = L.rtc_last_error()
    assert b"rtc_render_first_hit_async" in msg and b"null" in msg
