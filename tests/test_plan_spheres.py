"""The sphere split in the launch planner (rtc_plan.h sphere_split), on the CPU through rtc_plan_sim_*:
which launches that render spheres take the split launch (tile cull, sky pass, rtc_render_chain) and which keep the
one-lane-per-pixel kernel, that a scene without spheres plans exactly as before, that sequences mixing both kinds of
launch stay race free under tests/test_plan.py's stream model, and the upload gate's probe (bounce_hit_share with
spheres).  Reference: calculateRayCollision's sphere loop, raytracing.c:219-228; the seam main.c:263-304."""
from __future__ import annotations

import random

import pytest

import raytracingc_amd as rt
from conftest import load_tris, scene_spheres
from raytracingc_amd._abi import RtcRenderDesc
from sphere_scenes import open5
from test_plan import CAMS, ENVS, OVERLAP, Scenario, _random_launch

SPLIT = rt.RTC_F_SPLIT_SPHERES
STREAM = 0x7f001000


def _desc(W, H, spp, row_start=0, stride=1, band=0, flags=0, tonly=0):
    return RtcRenderDesc(W, H, spp, 10, tonly, row_start, stride, flags, band)


def _sim(tri_count, spheres=None, gate=1):
    sc = Scenario(tri_count)
    if spheres is not None:
        assert sc.L.rtc_plan_sim_set_spheres(sc.h, spheres, gate) == 0
    return sc


def _kernels(sc, d, colors=0x1000):
    sc.launch(d, STREAM, colors, 0, False, CAMS[0], ENVS[0])
    return [k for k, _ in sc.kernel_order()]


# (W, H, spp, rowStart, rowStride, rowBand, flags)
SHAPES = {"whole": (1920, 1080, 64, 0, 1, 0, 0), "whole_overlapped": (1920, 1080, 64, 0, 1, 0, OVERLAP),
          "small_share_overlapped": (1920, 1080, 64, 3, 8, 0, OVERLAP),
          "band_share_overlapped": (1920, 1080, 64, 8, 8, 8, OVERLAP), "small_frame": (96, 54, 8, 0, 1, 0, 0)}


@pytest.mark.parametrize("n", [1, 32])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sphere_launch_plans_the_split(n, shape):
    d = _desc(*SHAPES[shape])
    sc = _sim(120, n, 1)
    try:
        ks = _kernels(sc, d)
        assert "tile_cull" in ks and "sky" in ks and "chain" in ks and "render" not in ks, ks
    finally:
        sc.close()


@pytest.mark.parametrize("case,n,gate,flags", [
    ("33_spheres", 33, 1, 0), ("33_spheres_forced", 33, 1, SPLIT), ("gate_off", 5, 0, 0),
    ("no_coop", 5, 1, rt.RTC_F_NO_COOP), ("no_coop_forced", 5, 1, rt.RTC_F_NO_COOP | SPLIT),
    ("debug", 5, 1, rt.RTC_F_DEBUG_BOUNCES), ("debug_forced", 5, 0, rt.RTC_F_DEBUG_BOUNCES | SPLIT),
    ("no_tile_cull", 5, 1, rt.RTC_F_NO_TILE_CULL), ("no_tile_cull_forced", 5, 1, rt.RTC_F_NO_TILE_CULL | SPLIT),
    ("no_reorder", 5, 1, rt.RTC_F_NO_REORDER)])
@pytest.mark.parametrize("overlap", [0, OVERLAP])
def test_sphere_launch_keeps_the_pixel_kernel(case, n, gate, flags, overlap):
    sc = _sim(120, n, gate)
    try:
        ks = _kernels(sc, _desc(1920, 1080, 64, flags=flags | overlap))
        assert "render" in ks and "chain" not in ks and "sky" not in ks, ks
    finally:
        sc.close()


def test_flag_forces_the_split_past_the_gate():
    sc = _sim(120, 5, 0)
    try:
        for args in SHAPES.values():
            ks = _kernels(sc, _desc(*args[:6], args[6] | SPLIT))
            assert "chain" in ks and "sky" in ks and "render" not in ks, ks
            assert "render" in _kernels(sc, _desc(*args))  # and without the flag the gate holds
    finally:
        sc.close()


def test_triangles_only_launch_on_a_sphere_scene_plans_as_before():
    """trianglesOnly renders no sphere: the split launch whatever the gate says, as on a scene without spheres."""
    sc = _sim(120, 5, 0)
    try:
        ks = _kernels(sc, _desc(1920, 1080, 64, tonly=1))
        assert "chain" in ks and "render" not in ks
    finally:
        sc.close()


def _trace(sc, launches):
    out = []
    for d, stream, colors, accum, seg, cam, env in launches:
        info = sc.launch(d, stream, colors, accum, seg, cam, env)
        out.append((tuple(sc.last_ops), tuple(sorted(info.items()))))
    out.append(tuple((a[1], a[2], a[3], a[4], a[5], a[7], a[8]) for a in sc.accesses))
    return out


@pytest.mark.parametrize("tonly", [0, 1])
def test_zero_spheres_plans_identically(tonly):
    """n = 0 through the setter (either gate value) gives the plans of a sim that never called it, op for op and
    footprint for footprint, over a random sequence of launches."""
    rng = random.Random(77)
    launches = []
    for _ in range(40):
        d = _random_launch(rng, rng.choice([(1920, 1080), (640, 360), (256, 256), (3840, 2160)]))
        d.trianglesOnly = tonly
        seg = not (d.flags & OVERLAP) and rng.random() < 0.2
        launches.append((d, STREAM, rng.choice([0x1000, 0x2000]), 0, seg, rng.choice(CAMS), rng.choice(ENVS)))
    traces = []
    for spheres, gate in [(None, 0), (0, 0), (0, 1)]:
        sc = _sim(300, spheres, gate)
        try:
            traces.append(_trace(sc, launches))
        finally:
            sc.close()
    assert traces[0] == traces[1] == traces[2]


def _mixed_launch(rng, shape):
    d = _random_launch(rng, shape)
    d.trianglesOnly = int(rng.random() < 0.4)
    if rng.random() < 0.3:
        d.flags |= SPLIT
    if rng.random() < 0.1:
        d.flags |= rt.RTC_F_NO_COOP
    return d


@pytest.mark.parametrize("tri_count", [120, 5208, 0])
@pytest.mark.parametrize("seed", range(3))
def test_mixed_sphere_sequences_are_race_free(seed, tri_count):
    """tests/test_plan.py's checker over random sequences on one scene that mix launches rendering its spheres (split by
    the gate, forced by the flag, or on the pixel kernel) with triangle-only launches -- and the same on a scene of
    spheres alone (0 triangles: no mask words, no triangle records): no unordered pair of conflicting kernels."""
    rng = random.Random(4200 + 17 * seed + tri_count)
    shapes = [(1920, 1080), (3840, 2160), (640, 360), (256, 256), (1000, 700)]
    split_launches = 0
    for _ in range(30):
        sc = _sim(tri_count, rng.choice([1, 5, 32, 33]), rng.choice([0, 1, 1]))
        streams = [rng.choice([0, STREAM, 0x7f002000])]
        if rng.random() < 0.3:
            streams.append(rng.choice([0, 0x7f003000]))
        try:
            shape = rng.choice(shapes)
            for _ in range(24):
                if rng.random() < 0.15:
                    shape = rng.choice(shapes)
                d = _mixed_launch(rng, shape)
                seg = not (d.flags & OVERLAP) and rng.random() < 0.2
                colors = rng.choice([0x1000, 0x2000, 0x3000])
                accum = rng.choice([0, 0, 0, 0x9000 + colors])
                sc.launch(d, rng.choice(streams), colors, accum, seg, rng.choice(CAMS), rng.choice(ENVS))
                ks = [k for k, _ in sc.kernel_order()]
                split_launches += (not d.trianglesOnly) and "chain" in ks
            hz = sc.hazards()
            assert not hz, f"unordered conflicting kernels: {hz}"
        finally:
            sc.close()
    assert split_launches > 50  # the sequences do exercise sphere launches on the split path


def test_setter_rejects_bad_arguments():
    sc = Scenario(12)
    try:
        assert sc.L.rtc_plan_sim_set_spheres(None, 1, 1) == rt.RTC_EINVAL
        assert sc.L.rtc_plan_sim_set_spheres(sc.h, -1, 1) == rt.RTC_EINVAL
    finally:
        sc.close()


# bounce_hit_share(tris) before the probe learnt about spheres (float32 values of the triangle-only probe)
SHARES_BEFORE = {"fsuzane": 0.21826171875, "ultracomplex": 0.01708984375, "cube": 0.0}


@pytest.mark.parametrize("name", sorted(SHARES_BEFORE))
def test_triangle_hit_share_unchanged(name):
    tris, _ = load_tris(name)
    assert rt.bounce_hit_share(tris) == SHARES_BEFORE[name]
    # no spheres: the extended probe is the triangle-only one, draw for draw
    assert rt.bounce_hit_share(tris, scene_spheres(name)) == SHARES_BEFORE[name]


def test_hit_share_with_spheres_orders_closed_and_open_scenes():
    box, _ = load_tris("default")
    model, _ = load_tris("ultracomplex")
    closed = rt.bounce_hit_share(box, scene_spheres("default"))
    opened = rt.bounce_hit_share(model, open5())
    assert 0.0 <= opened < closed <= 1.0
    # spheres alone (no triangles): rays leave a sphere outwards and can only hit another one
    alone = rt.bounce_hit_share(None, open5())
    assert 0.0 <= alone < closed
