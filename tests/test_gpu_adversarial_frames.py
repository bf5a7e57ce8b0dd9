"""Whole frames of the adversarial scenes (tests/adversarial_scenes.py) on every route of the renderer, against the CPU
oracle: NaN positions equal, every other float of the accumulator bit-equal, the u8 frame equal, and the segment count
equal where the launch counts.  The routes are the item-record routes of tests/test_gpu_item_records.py (the split launch
joined with deferred and in-kernel sums, hoisted, pipelined) and the launches without the tile cull, without the split
launch (coop off) and without the cluster cull.  On gfx950 and x86 a NaN's sign bit may differ: NaN positions are compared,
not NaN bits."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import raytracingc_amd as rt
from adversarial_scenes import SCENES
from raytracingc_amd._abi import RtcRenderDesc
from test_gpu_item_records import ROUTES as ITEM_ROUTES

pytestmark = pytest.mark.gpu

ROUTES = {k: ITEM_ROUTES[k] for k in ("joined_deferred", "joined_inline", "hoisted", "pipelined")}
ROUTES.update(no_tile_cull=dict(tile_cull=False), no_coop=dict(coop=False), no_cluster_cull=dict(cluster_cull=False))
SHAPES = {"48x40x6": (48, 40, 6), "33x17x3": (33, 17, 3)}
MAX_BOUNCE = 4
NAMES = sorted(n for n in SCENES if not n.startswith("counts_") or n in ("counts_1", "counts_8", "counts_9", "counts_65"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(name, shape):
    """The oracle's (u8, floats, segments) of the frame, computed once and left unchanged."""
    tris, cam, _ = SCENES[name]
    W, H, spp = SHAPES[shape]
    col, acc, seg = orc.render(tris, None, rt.default_scene(), cam, RtcRenderDesc(W, H, spp, MAX_BOUNCE, 1, 0, 1, 0, 0),
                               threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


@functools.lru_cache(maxsize=None)
def _device_scene(name):
    return rt.DeviceScene(SCENES[name][0], None)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", NAMES)
def test_frame_matches_oracle(name, shape, route, gpu_available):
    import torch

    _, cam, _ = SCENES[name]
    W, H, spp = SHAPES[shape]
    scene = rt.default_scene()
    cfg = rt.RenderConfig(W, H, spp, MAX_BOUNCE, True, **ROUTES[route])
    ocol, oacc, oseg = _oracle(name, shape)
    nan = np.isnan(oacc)
    ds = _device_scene(name)
    st = torch.cuda.current_stream().cuda_stream
    # the route itself (a launch that counts segments is always a joined one), then the same launch counting
    for counters in (False, True):
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
        torch.cuda.synchronize()
        ds.render_rows_async(scene, cam, cfg, out.data_ptr(), acc.data_ptr(), seg.data_ptr() if counters else None, st)
        torch.cuda.synchronize()
        col, a = out.cpu().numpy(), acc.cpu().numpy()
        what = f"{name} {shape} {route} counters={counters}"
        assert np.array_equal(np.isnan(a), nan), f"{what}: NaN positions differ ({int(np.isnan(a).sum())} vs {int(nan.sum())})"
        bad = int(((_bits(a) != _bits(oacc)) & ~nan).any(-1).sum())
        assert bad == 0, f"{what}: {bad} pixels' accumulator bits differ"
        assert np.array_equal(col, ocol), f"{what}: {int((col != ocol).any(-1).sum())} u8 pixels differ"
        if counters:
            assert int(seg.cpu().numpy()[0]) == oseg, f"{what}: segments"
