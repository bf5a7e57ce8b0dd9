"""The premises of tests/test_gpu_occluded.py, from the CPU oracle alone
(tests/occlusion_reference.py): the two forms of the definition agree (closest.didHit && closest.dst < L against "some
primitive reports a hit with dst < L and dst < 999999"), the limit sets do what the GPU test leans on (a tie occludes
nothing, one ulp above occludes every hit, the median splits the hits, the odd limits occlude nothing) and the segments
have both answers.  Reference: calculateRayCollision (raytracing.c:216-240), raySphere / rayTriangle
(:162-214)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import occlusion_reference as oc
import trace_rays_reference as tr

BRUTE_CASES = ("suze", "counts_9", "chunks", "slivers", "default")
# the cases whose hit depths are not all alike: the median of the hits' depths then has hits on both sides
# (test_median_splits_the_hits checks exactly this list against the reference)
MEDIAN_CASES = tuple(sorted(tr.REPLAY))


@functools.lru_cache(maxsize=None)
def _hits(name):
    tris, spheres, tonly, _ = tr.geometry(name)
    return oc.primitive_hits(tris, spheres, tonly, tr.replay(name))


@pytest.mark.parametrize("limit", oc.LIMITS)
@pytest.mark.parametrize("name", BRUTE_CASES)
def test_the_two_forms_agree(name, limit):
    tris, spheres, tonly, _ = tr.geometry(name)
    rays, lim = tr.replay(name), oc.case_limits("replay", name, limit)
    want = oc.expected(tris, spheres, tonly, rays, lim)
    got = oc.brute(tris, spheres, tonly, rays, lim, _hits(name))
    print(f"{name} {limit}: {len(rays)} rays, {int(want.sum())} occluded")
    assert np.array_equal(want, got)
    assert np.array_equal(want, oc.case_occluded("replay", name, limit))


@pytest.mark.parametrize("name", sorted(tr.REPLAY))
def test_limit_set_premises(name):
    """tie: none; above: exactly the hits; below: none (one ulp under the closest hit); none / inf / 999999 / 1e30: the
    hits; short: fewer than median."""
    hits = tr.REPLAY[name][1]
    count = {k: int(oc.case_occluded("replay", name, k).sum()) for k in oc.LIMITS}
    print(name, count)
    assert count["tie"] == 0 and count["below"] == 0
    assert count["above"] == count["none"] == count["inf"] == count["999999"] == count["1e30"] == hits
    assert count["short"] <= count["median"] <= hits


@pytest.mark.parametrize("name", MEDIAN_CASES)
def test_median_splits_the_hits(name):
    e, occ = tr.case_expected("replay", name), oc.case_occluded("replay", name, "median")
    hit = e["prim"] != -1
    print(f"{name}: {int(hit.sum())} hits, {int(occ.sum())} below the median")
    assert (occ & hit).any() and (~occ & hit).any() and not (occ & ~hit).any()


@pytest.mark.parametrize("name", BRUTE_CASES)
def test_odd_limits(name):
    """NaN, +-0, -1, -inf, EPSILON and 1e-30 occlude nothing (no reference test reports dst < EPSILON); at
    nextafter(EPSILON) whatever the brute form says."""
    tris, spheres, tonly, _ = tr.geometry(name)
    lim = oc.case_limits("replay", name, "odd")
    got = oc.brute(tris, spheres, tonly, tr.replay(name), lim, _hits(name))
    with np.errstate(invalid="ignore"):
        assert not got[~(lim > oc.EPSILON)].any()
    assert np.array_equal(got, oc.case_occluded("replay", name, "odd"))


@pytest.mark.parametrize("name", ["chunks", "default", "box_mirror"])
def test_segments(name):
    """Line of sight: dir = end - pos, tMax = 1.  chunks has both answers."""
    tris, spheres, tonly, _ = tr.geometry(name)
    rays, lim = oc.segments(name)
    assert (lim == 1).all() and len(rays) == len(tr.replay(name))
    occ = oc.expected(tris, spheres, tonly, rays, lim)
    print(f"{name}: {len(rays)} segments, {int(occ.sum())} occluded")
    if name == "chunks":
        assert occ.any() and (~occ).any()
        assert np.array_equal(occ, oc.brute(tris, spheres, tonly, rays, lim))
