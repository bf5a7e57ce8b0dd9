"""The ray order's key without a GPU (include/rtc.h): rtc_ray_keys_host against the numpy float32 statement of
tests/ray_order_reference.py, bit for bit, on the designed sets; and the premise the feature rests on -- sorting a permuted
frame's rays by that key gives 64-ray groups at least as coherent as raster order's, measured with the oracle's rayTriangle
(raytracing.c:186-214) through tests/primary_rays.hit_table."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import ray_order_reference as ro
import raytracingc_amd as rt
from conftest import load_tris
from primary_rays import hit_table, launch_rays

# the coherence premise's frame: the golden camera on ultracomplex at the issue's size (the first inequality holds there)
FRAME = (480, 270)
PERM_SEED = 2024  # tools/trace_paths_probe.py's


@pytest.mark.parametrize("name", sorted(ro.DESIGNED))
def test_host_keys_equal_the_numpy_statement(name):
    make, lo, hi = ro.DESIGNED[name]
    rays = make()
    want = ro.keys(rays, lo, hi)
    got = rt.ray_keys_host(rays, lo, hi)
    bad = np.flatnonzero(got != want)
    print(f"{name}: {len(rays)} rays, {len(np.unique(want))} distinct keys, {len(bad)} differ")
    assert got.dtype == np.uint32 and got.shape == (len(rays),)
    assert len(bad) == 0, (name, rays[bad[:4]], got[bad[:4]], want[bad[:4]])
    assert int(got.max()) < 1 << 30 and int(want.max()) < 1 << 30


def test_designed_sets_reach_what_they_are_for():
    """The sets' premises: both clamps and every cell of an axis among the origins, every octant and both ends of q among
    the directions, the random set at 10,000 rays."""
    k = ro.keys(ro.origin_set(), ro.LO, ro.HI)
    cell = k >> 15
    for a in range(3):
        c = sum(((cell >> (3 * b + a)) & 1) << b for b in range(5))
        assert set(np.unique(c)) == set(range(32)), a
    d = ro.keys(ro.direction_set(), ro.LO, ro.HI)
    assert set(np.unique((d >> 12) & 7)) == set(range(8))
    assert {0, 63} <= set(np.unique(d & 63)) and {0, 63} <= set(np.unique((d >> 6) & 63))
    assert len(np.unique(d & 63)) == 64  # every bin of q(px): the exactly integral p * 64
    f = ro.keys(ro.flat_set(), ro.FLAT_LO, ro.FLAT_HI)
    cy = sum((((f >> 15) >> (3 * b + 1)) & 1) << b for b in range(5))
    assert not cy.any(), "a flat axis gives cell 0"
    assert len(ro.random_set()) == 10000


def test_particular_values():
    """A few keys by hand: the box's corner cells, the octant bits, -0 and NaN as not negative, the zero direction."""
    lo, hi = [0, 0, 0], [32, 32, 32]
    key = lambda p, d: int(rt.ray_keys_host(ro.make_rays(p, d), lo, hi)[0])  # noqa: E731
    assert key([0, 0, 0], [0, 0, 1]) == 0
    assert key([0, 0, 0], [1, 0, 0]) == 63 and key([0, 0, 0], [0, 1, 0]) == 63 << 6
    assert key([0, 0, 0], [-1, 0, 0]) == 63 | 1 << 12 and key([0, 0, 0], [0, 0, -1]) == 4 << 12
    assert key([0, 0, 0], [-0.0, -0.0, 1]) == 0 and key([0, 0, 0], [np.nan, 0, 1]) == 0
    assert key([0, 0, 0], [0, 0, 0]) == 0 and key([0, 0, 0], [np.inf, 1, 1]) == 0
    assert key([1, 0, 0], [0, 0, 1]) == 1 << 15 and key([0, 1, 0], [0, 0, 1]) == 2 << 15
    assert key([0, 0, 1], [0, 0, 1]) == 4 << 15 and key([2, 0, 0], [0, 0, 1]) == 8 << 15
    assert key([31.5, 99, np.inf], [0, 0, 1]) == 0x7FFF << 15
    assert key([-5, np.nan, -np.inf], [0, 0, 1]) == 0
    assert key([0, 0, 0], [1, 1, 2]) == 16 | 16 << 6  # px = py = 0.25


def test_python_surface_checks_its_arguments():
    with pytest.raises(ValueError):
        rt.ray_keys_host(np.zeros((2, 5), np.float32), [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError):
        rt.ray_keys_host(np.zeros((2, 6), np.float32), [0, 0], [1, 1, 1])
    assert rt.ray_keys_host(np.zeros((0, 6), np.float32), [0, 0, 0], [1, 1, 1]).shape == (0,)
    assert rt.lib().rtc_ray_keys_host(None, 4, None, None, None) == rt.RTC_EINVAL
    assert b"rtc_ray_keys_host" in rt.lib().rtc_last_error()


@functools.lru_cache(maxsize=None)
def _frame():
    """(rays in raster order, hitting ray or not, the scene's box) of the golden camera's frame on ultracomplex."""
    tris, _ = load_tris("ultracomplex")
    rays = launch_rays(rt.camera_basis(), rt.RenderConfig(FRAME[0], FRAME[1], 0, 0, True))
    hit = hit_table(orc.ray_triangle, tris, rays)[0].any(1)
    v = np.concatenate([np.stack([tris[k][c] for c in "xyz"], 1) for k in ("posA", "posB", "posC")])
    return rays, hit, v.min(0).astype(np.float32), v.max(0).astype(np.float32)


def test_the_key_restores_coherence():
    """The share of 64-ray groups that hold a ray which hits a triangle: raster order, the frame permuted (seed 2024), and
    the permuted frame stable-sorted by the host keys in the scene's box.  The ordered share must not exceed raster's, and
    the permuted share is at least five times the ordered one.  (At 1080p, in float64: 5.2 %, 90.9 %, 4.7 %.)"""
    rays, hit, lo, hi = _frame()
    perm = np.random.default_rng(PERM_SEED).permutation(len(rays))
    keys = rt.ray_keys_host(rays[perm], lo, hi)
    order = np.argsort(keys, kind="stable")
    raster, permuted, ordered = ro.group_share(hit), ro.group_share(hit[perm]), ro.group_share(hit[perm][order])
    print(f"{FRAME[0]}x{FRAME[1]}: {int(hit.sum())} of {len(rays)} rays hit; {len(np.unique(keys))} distinct keys; groups "
          f"with a hit: raster {raster:.4f}, permuted {permuted:.4f}, ordered {ordered:.4f}")
    assert 0 < hit.sum() < len(rays)
    assert ordered <= raster
    assert permuted >= 5 * ordered

