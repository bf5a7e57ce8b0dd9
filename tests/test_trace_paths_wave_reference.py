"""The premise of RTC_F_WAVE_PER_RAY without a GPU, from oracle.binding.calc_path alone, on every set of
tests/test_gpu_trace_paths_wave.py (tests/trace_paths_wave_sets.all_sets), for every ray and every sample the GPU tests
run (each set at the largest spp it is run at): a sample's m-th hit draws exactly 7 values (RandomDiretion's six and the
roulette's one, raytracing.c:274, 285; moremath.c:97-108) and a miss none, so the RNG state after a sample is the state
before it advanced by 7 * hits steps of RandomValue's LCG (moremath.c:89-95) -- which is why every sample of a ray starts at
the caller's seed advanced by a multiple of 7 draws.  And the sets hold what that file relies on: box_mirror's and box_gloss'
samples make exactly maxBounce hits, the designed miss rays none, suze[::20] both."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import raytracingc_amd as rt
import trace_paths_reference as tp
import trace_paths_wave_sets as ws

LCG_A, LCG_C = 747796405, 2891336453  # moremath.c:91
SETS = {label: rest for label, *rest in ws.all_sets()}


@functools.lru_cache(maxsize=None)
def lcg_maps(steps):
    """uint64 [steps + 1, 2]: row k is (a, c) with k steps of s = s * A + C (mod 2^32) equal to s * a + c, built one step
    at a time."""
    rows, a, c = [], 1, 0
    for _ in range(steps + 1):
        rows.append((a, c))
        a, c = a * LCG_A & 0xFFFFFFFF, (c * LCG_A + LCG_C) & 0xFFFFFFFF
    return np.array(rows, np.uint64)


def lcg_advance(state, steps):
    """uint32 [n]: state[i] after steps[i] LCG steps."""
    m = lcg_maps(int(steps.max(initial=0)))[steps]
    return ((np.asarray(state, np.uint64) * m[:, 0] + m[:, 1]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def samples_of(tris, spheres, tonly, rays, seeds, max_bounce, samples):
    """Per sample of the chain: (state before, state after, calls, hits) for every ray."""
    tris, spheres = ws.records(tris, spheres)
    rays = np.ascontiguousarray(rays)
    state = np.array(seeds, np.uint32)
    with np.errstate(all="ignore"):
        for _ in range(samples):
            _, after, calls, ncalls = orc.calc_path(tris, spheres, rt.default_scene(), int(tonly), rays, state,
                                                    np.full(len(rays), max_bounce, np.int32))
            last = calls[np.arange(len(rays)), np.maximum(ncalls - 1, 0)]["winner"]
            hits = ncalls - ((ncalls > 0) & (last == -1))  # (maxBounce <= 0: no call, no hit)
            yield state, after, ncalls, hits
            state = after


def _named(name, rays, seeds, max_bounce, samples):
    tris, spheres, tonly, _ = tp.geometry(name)
    return samples_of(tris, spheres, tonly, rays, seeds, max_bounce, samples)


@pytest.mark.parametrize("label", sorted(SETS))
def test_a_sample_advances_the_state_by_seven_draws_per_hit(label):
    tris, spheres, tonly, rays, seeds, max_bounce, spp = SETS[label]
    assert 0 < len(rays) <= 2560 and len(seeds) == len(rays)
    done = 0
    for before, after, ncalls, hits in samples_of(tris, spheres, tonly, rays, seeds, max_bounce, spp):
        assert (hits >= 0).all() and (hits <= max(max_bounce, 0)).all() and (ncalls - hits <= 1).all()
        assert (ncalls >= 1).all() or max_bounce <= 0
        assert np.array_equal(after, lcg_advance(before, 7 * hits.astype(np.int64))), (label, done)
        done += 1
    assert done == spp


def test_the_lcg_maps_are_the_steps():
    s = tp.hash_seeds(64).astype(np.uint64)
    want = s.copy()
    for _ in range(9):
        want = (want * np.uint64(LCG_A) + np.uint64(LCG_C)) & np.uint64(0xFFFFFFFF)
    assert np.array_equal(lcg_advance(s, np.full(64, 9)), want.astype(np.uint32))
    assert np.array_equal(lcg_advance(s, np.zeros(64, np.int64)), s.astype(np.uint32))


@pytest.mark.parametrize("name, max_bounce", sorted({(n, mb) for n, _, mb in ws.WINDOW_CASES if n != "box_diffuse_T"}))
def test_shiny_boxes_make_exactly_max_bounce_hits(name, max_bounce):
    rays = ws.box_rays(name)
    spp = max(s for n, s, mb in ws.WINDOW_CASES if (n, mb) == (name, max_bounce))
    for _, _, ncalls, hits in _named(name, rays, tp.pixel_seeds(len(rays)), max_bounce, spp):
        assert (hits == max_bounce).all() and (ncalls == max_bounce).all()


def test_the_diffuse_box_mixes_hit_counts():
    rays = ws.box_rays("box_diffuse_T")
    hits = np.stack([h for _, _, _, h in _named("box_diffuse_T", rays, tp.pixel_seeds(len(rays)), 40, 130)])
    # a closed box: every sample hits; 130 samples of about three hits each walk through several windows of 64 lanes
    assert hits.min() >= 1 and len(np.unique(hits)) >= 8 and 2 < hits.mean() < 8
    assert (hits.sum(0) > 3 * 64).all()


def test_the_miss_rays_hit_nothing():
    rays = ws.miss_rays()
    seeds = tp.hash_seeds(len(rays))
    for before, after, ncalls, hits in _named(ws.MISS_SCENE, rays, seeds, tp.MAX_BOUNCE, 3):
        assert (ncalls == 1).all() and (hits == 0).all() and np.array_equal(after, seeds)
    for spp in ws.MISS_SPPS:
        radiance, state, seg = ws.miss_expected(spp)
        assert seg == spp * len(rays) and np.array_equal(state, seeds)
    # the continuation's accumulators: a row that no add moves (1e30, inf, nan) beside rows every add moves (-0, 0)
    acc0 = ws.miss_acc0()
    radiance, _, seg = ws.miss_expected(130, 1)
    assert seg == 129 * len(rays)
    moved = (radiance.view(np.uint32) != acc0.view(np.uint32)).any(1)
    assert not moved[np.arange(65) % 5 < 3].any() and moved[np.arange(65) % 5 >= 3].all()


def test_suze_holds_hits_and_misses():
    rays, seeds = ws.suze_rays()
    assert len(rays) == 128
    _, _, ncalls, hits = next(_named("suze", rays, seeds, tp.MAX_BOUNCE, 1))
    assert (hits == 0).sum() > 20 and (hits >= 1).sum() > 5
