"""The adversarial scenes (tests/adversarial_scenes.py) are not vacuous: with the CPU oracle alone, the ties are ties, the
NaN normals give NaN pixels, the `sane` switch has hit triangles on both sides, the oversized and degenerate triangles are
never the closest hit and their frames still hold geometry -- every cap the GPU tests (tests/test_gpu_primary_cull.py,
tests/test_gpu_adversarial_frames.py, tests/test_gpu_cluster.py) rely on.  A scene that misses a cap is changed, not the
cap."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import raytracingc_amd as rt
from adversarial_scenes import (COUNTS, DEGENERATE, NAN_NORMALS, OVERSIZED, SANE_PRODUCT, SCENES, cluster_order)
from primary_rays import hit_table, launch_rays, prep_flags
from raytracingc_amd._abi import RAY_DT, RtcRenderDesc

TIES = ("ties_axis", "ties_tilted", "ties_rotated")
FRAME = (48, 40, 6, 4)  # tests/test_gpu_adversarial_frames.py: width, height, spp, maxBounce


@functools.lru_cache(maxsize=None)
def table(name, W, H):
    """(recorded, dst, rays) of the scene's W x H frame: oracle.ray_triangle on every (pixel, triangle) pair."""
    tris, cam, _ = SCENES[name]
    rays = launch_rays(cam, rt.RenderConfig(W, H, 1, 4, True))
    rec, dst = hit_table(orc.ray_triangle, tris, rays)
    return rec, dst, rays


def nearest_ties(rec, dst):
    """Per ray: the two lowest triangle indices among the recorded hits at the bit-equal smallest dst (or -1, -1)."""
    d = np.where(rec, dst, np.float32(np.inf))
    near = d.min(1)
    tied = rec & (d == near[:, None])
    has = tied.sum(1) >= 2
    first = np.argmax(tied, 1)
    rest = tied.copy()
    rest[np.arange(len(rest)), first] = False
    second = np.argmax(rest, 1)
    return np.where(has, first, -1), np.where(has, second, -1)


def cluster_of(tris):
    order = cluster_order(tris)
    c = np.empty(len(tris), np.int64)
    c[order] = np.arange(len(order)) // 8
    return c


def test_scene_table_is_as_specified():
    assert all(len(t) <= 64 or n == "chunks" or n.startswith("counts_") for n, (t, _, _) in SCENES.items())
    assert len(SCENES["chunks"][0]) > 256 and [len(SCENES[f"counts_{n}"][0]) for n in COUNTS] == list(COUNTS)
    for name, (tris, cam, note) in SCENES.items():
        m = np.stack([tris["mat"]["color"][c] for c in "xyz"] + [tris["mat"]["emissionStrength"], tris["mat"]["smoothness"]], 1)
        assert len(np.unique(m, axis=0)) == len(tris), f"{name}: two triangles share a material"


@pytest.mark.parametrize("name", TIES)
def test_primary_ties(name):
    tris, cam, _ = SCENES[name]
    rec, dst, _ = table(name, 32, 32)
    lo, hi = nearest_ties(rec, dst)
    n = int((lo >= 0).sum())
    cl = cluster_of(tris)
    later = int(((lo >= 0) & (cl[lo] > cl[hi])).sum())
    print(f"{name}: {n} of {int(rec.any(1).sum())} geometry pixels have a tied nearest hit; lower index in the later "
          f"cluster for {later}")
    assert n >= 100


def test_a_tie_has_its_lower_index_in_the_later_cluster():
    best = 0
    for name in TIES:
        tris, _, _ = SCENES[name]
        rec, dst, _ = table(name, 32, 32)
        lo, hi = nearest_ties(rec, dst)
        cl = cluster_of(tris)
        best = max(best, int(((lo >= 0) & (cl[lo] > cl[hi])).sum()))
    assert best >= 100


def _f32_normalized(v):
    f = np.float32
    sq = (v * v).astype(f)
    ss = ((sq[:, 0] + sq[:, 1]).astype(f) + sq[:, 2]).astype(f)
    inv = (1.0 / np.sqrt(ss.astype(np.float64)).astype(f).astype(np.float64)).astype(f)
    return (v * inv[:, None]).astype(f)


@pytest.mark.parametrize("name", TIES)
def test_first_bounce_ties(name):
    """The first sample's first bounce of every pixel of the test frame whose primary ray records a hit (raytracing.c:
    270-281 in float32: the pixel's seed x + y * width, diffuse = normalized(N + randomDirection), the reflection, their
    lerp by the smoothness), traced through oracle.ray_triangle: tied nearest hits among them."""
    f = np.float32
    tris, cam, _ = SCENES[name]
    W, H = FRAME[:2]
    rec, dst, rays = table(name, W, H)
    d = np.where(rec, dst, f(np.inf))
    win, geo = np.argmin(d, 1), rec.any(1)
    px = np.flatnonzero(geo)
    t = tris[win[px]]
    dirs = np.stack([rays["dir"][c][px] for c in "xyz"], 1)
    pos = np.stack([rays["pos"][c][px] for c in "xyz"], 1)
    N = np.stack([t["normal"][c] for c in "xyz"], 1)
    hitp = (pos + (dirs * d[px, win[px]][:, None]).astype(f)).astype(f)
    rd = orc.random_sequences(px.astype(np.uint32), 1)[2][:, 0, :]  # (seed = x + y * width = the pixel's index)
    diffuse = _f32_normalized((N + rd).astype(f))
    dn = (dirs * N).astype(f)
    dn = ((dn[:, 0] + dn[:, 1]).astype(f) + dn[:, 2]).astype(f)
    spec = (dirs - (N * (2.0 * dn.astype(np.float64)).astype(f)[:, None]).astype(f)).astype(f)
    s = t["mat"]["smoothness"][:, None]
    bdir = ((diffuse * (f(1) - s)).astype(f) + (spec * s).astype(f)).astype(f)
    brays = np.zeros(len(px), RAY_DT)
    for k, c in enumerate("xyz"):
        brays["pos"][c], brays["dir"][c] = hitp[:, k], bdir[:, k]
    brec, bdst = hit_table(orc.ray_triangle, tris, brays)
    lo, _ = nearest_ties(brec, bdst)
    n = int((lo >= 0).sum())
    print(f"{name}: {n} of {int(brec.any(1).sum())} first bounces that hit have a tied nearest hit ({len(px)} bounces)")
    assert n >= 20


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    tris, cam, _ = SCENES[name]
    W, H, spp, mb = FRAME
    col, acc, seg = orc.render(tris, None, rt.default_scene(), cam, RtcRenderDesc(W, H, spp, mb, 1, 0, 1, 0, 0), threads=8)
    return col, acc, seg


def test_nan_normals_render_nan_pixels():
    tris, cam, _ = SCENES["bad_normals"]
    W, H = FRAME[:2]
    rec, dst, _ = table("bad_normals", W, H)
    win = np.argmin(np.where(rec, dst, np.float32(np.inf)), 1)
    through = rec.any(1) & np.isin(win, NAN_NORMALS["bad_normals"])
    _, acc, _ = oracle_frame("bad_normals")
    nan = np.isnan(acc).any(-1).reshape(-1)
    print(f"bad_normals: {int(nan.sum())} of {W * H} pixels are NaN, {int(through.sum())} primary rays end on a NaN normal")
    # a triangle of area 0.55 at z = 3.5 covers 0.55 / (2 * 3.5 / 40)^2 = 18 pixels of the frame; there are two
    assert int(through.sum()) >= 20 and nan[through].all()


@pytest.mark.parametrize("name", [n for n, s in SCENES.items() if "sane straddle" in s[2]])
def test_sane_switch_has_hit_triangles_on_both_sides(name):
    tris, cam, _ = SCENES[name]
    sane, never, ed = prep_flags(tris, cam.origin)
    for W, H in ((64, 40), (33, 17)):
        rec, _, _ = table(name, W, H)
        hit = rec.any(0)
        # triangles 0 and 1: |AB|_1 |AC|_1 2 % below and above the switch
        below, above = hit & sane & ~never, hit & ~sane & ~never
        print(f"{name} {W}x{H}: hit and sane {np.flatnonzero(below)}, hit and not sane {np.flatnonzero(above)}; "
              f"ed / 2.5e-4 of 0, 1 = {ed[0] / 2.5e-4:.4f}, {ed[1] / 2.5e-4:.4f}")
        assert below[0] and above[1]
        assert 0.97 < ed[0] / 2.5e-4 < 1.0 < ed[1] / 2.5e-4 < 1.03
    assert abs(SANE_PRODUCT * 4 * 9.006 * 2.0 ** -24 / 2.5e-4 - 1) < 1e-12


@pytest.mark.parametrize("name", sorted(set(OVERSIZED) | set(DEGENERATE)))
def test_oversized_and_degenerate_triangles_are_never_the_hit(name):
    tris, cam, _ = SCENES[name]
    odd = list(OVERSIZED.get(name, ())) + list(DEGENERATE.get(name, ()))
    for W, H in ((FRAME[0], FRAME[1]), (64, 40), (33, 17)):
        rec, _, _ = table(name, W, H)
        geo = float(rec.any(1).mean())
        print(f"{name} {W}x{H}: {geo:.3f} of the pixels see geometry; recorded hits on {odd}: {rec[:, odd].sum(0)}")
        assert not rec[:, odd].any()
        assert geo >= 0.25


def test_filter_disabling_scenes_have_what_the_gpu_test_looks_for():
    """tests/test_gpu_primary_cull.py asserts `kept` everywhere for triangles that are not sane (and not `never`): they
    exist where the notes promise, and the `never` triangles of origin_in_plane are the three built so."""
    for name in ("mixed_scale", "mixed_scale_far_basis"):
        tris, cam, _ = SCENES[name]
        sane, never, _ = prep_flags(tris, cam.origin)
        assert (~sane & ~never).sum() >= 4 and not sane[list(OVERSIZED[name])].any()
    tris, cam, _ = SCENES["origin_in_plane"]
    _, never, _ = prep_flags(tris, cam.origin)
    assert list(np.flatnonzero(never)) == [0, 1, 2]
