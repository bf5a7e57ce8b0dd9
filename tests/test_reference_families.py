"""The CPU oracle (oracle/rtc_oracle.c) against the reference's own calcColor and calcDebugColor on the scene families the
later test modules built (tests/reference_calc.py: adversarial, boxes, materials, spheres, populations), read from the
committed tests/golden/kat_ref_<family>.npz.  No GPU, no reference checkout, no reference binary.

Per case the inputs are rebuilt and their sha256 compared with the fixture's first (a mismatch fails and says
"regenerate"); then colours are compared as uint32 bit patterns, NaN positions exactly (where the reference has a NaN any
NaN is accepted, the project's standing exception) and the seeds afterwards exactly, through oracle.binding.calc_color, its
debug mode and calc_path.

The non-vacuity tests assert on the fixture, i.e. on what the reference alone computed: hits in every scene, NaN and inf
records where the scenes are built for them, paths of exactly maxBounce calls in the boxes.  The tie counts state the tie
with the oracle's rayTriangle / raySphere per primitive on the records' own rays, not from any winner."""
from __future__ import annotations

import numpy as np
import pytest

import oracle.binding as orc
import raytracingc_amd as rt
import reference_calc as rc
from primary_rays import NO_HIT_DST, hit_table

SCENE = rt.default_scene()
CASES = [(f, c.name) for f in rc.FAMILIES for c in rc.cases(f)]
BY_NAME = {(f, c.name): c for f in rc.FAMILIES for c in rc.cases(f)}


def _ids(pairs):
    return [f"{f}-{n}" for f, n in pairs]


def test_fixture_holds_exactly_the_cases():
    for family in rc.FAMILIES:
        assert list(rc.fixture(family)) == [c.name for c in rc.cases(family)], \
            f"{family}: regenerate tests/golden/kat_ref_{family}.npz"
        has_debug = all(fx.debug_color is not None for fx in rc.fixture(family).values())
        assert has_debug == (family in rc.DEBUG_FAMILIES)


@pytest.mark.parametrize("family,name", CASES, ids=_ids(CASES))
def test_oracle_equals_reference(family, name):
    case = BY_NAME[family, name]
    rays, seeds, fx = rc.checked_inputs(family, case)
    mb = np.full(len(rays), case.max_bounce, np.int32)
    nan = np.isnan(fx.color)
    with np.errstate(all="ignore"):
        col, after = orc.calc_color(case.tris, case.spheres, SCENE, case.triangles_only, rays, seeds, mb)
        pcol, pafter, _, _ = orc.calc_path(case.tris, case.spheres, SCENE, case.triangles_only, rays, seeds, mb)
    for what, c, a in (("calc_color", col, after), ("calc_path", pcol, pafter)):
        assert np.array_equal(np.isnan(c), nan), f"{name} {what}: NaN positions differ"
        assert rc.differing(c, fx.color) == 0, f"{name} {what}: {rc.differing(c, fx.color)} records' colour bits differ"
        assert np.array_equal(a, fx.seed_after), f"{name} {what}: {int((a != fx.seed_after).sum())} seeds differ"
    if family in rc.DEBUG_FAMILIES:
        with np.errstate(all="ignore"):
            dcol, dafter = orc.calc_color(case.tris, case.spheres, SCENE, case.triangles_only, rays, seeds, mb, debug=True)
        assert np.array_equal(np.isnan(dcol), np.isnan(fx.debug_color)), f"{name} debug: NaN positions differ"
        assert rc.differing(dcol, fx.debug_color) == 0, f"{name} debug: colour bits differ"
        assert np.array_equal(dafter, fx.debug_seed_after), f"{name} debug: seeds differ"


# ---- non-vacuity: on the fixture alone ---------------------------------------------------------------------------------------
def _hit(fx):
    """Records whose path hit something: a hit draws (raytracing.c:274, :285), a miss does not."""
    return fx.seed_after != fx.pixels.astype(np.uint32)


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_every_scene_has_hits(family):
    hits = records = 0
    for name, fx in rc.fixture(family).items():
        h = int(_hit(fx).sum())
        if name in rc.EMPTY_CASES:
            assert h == 0, f"{name}: a hit in an empty scene"
        else:
            assert h >= 1, f"{name}: no record hits anything"
        hits += h
        records += len(fx.pixels)
    print(f"{family}: {hits} of {records} records hit")
    assert 10 * hits >= records, f"{family}: {hits} of {records} records hit"


def test_materials_reach_nan_and_inf():
    nan = sum(int(np.isnan(fx.color).any(-1).sum()) for fx in rc.fixture("materials").values())
    inf = sum(int(np.isinf(fx.color).any(-1).sum()) for fx in rc.fixture("materials").values())
    print(f"materials: {nan} NaN and {inf} inf records")
    assert nan >= 100 and inf >= 100


def test_bad_normals_reach_nan():
    fx = rc.fixture("adversarial")["bad_normals"]
    n = int(np.isnan(fx.color).any(-1).sum())
    print(f"bad_normals: {n} NaN records")
    assert n >= 1


TIES = [("adversarial", "ties_axis"), ("adversarial", "ties_tilted"), ("adversarial", "ties_rotated"),
        ("spheres", "tie_wide"), ("spheres", "tie_wide_spheres")]


def _first_call_candidates(case, rays):
    """float32 [records, primitives]: per primitive (the spheres first unless trianglesOnly, as calculateRayCollision walks
    them) the oracle's raySphere / rayTriangle dst on the record's ray where it reports a hit below 999999, else +inf."""
    n, cand = len(rays), []
    if not case.triangles_only:
        for i in range(len(case.spheres)):
            hit, dst, _ = orc.ray_sphere(rays, np.repeat(case.spheres[i:i + 1], n))
            cand.append(np.where((hit != 0) & (dst < NO_HIT_DST), dst, np.float32(np.inf)))
    if len(case.tris):
        rec, dst = hit_table(orc.ray_triangle, case.tris, rays)
        cand += list(np.where(rec, dst, np.float32(np.inf)).T)
    return np.stack(cand, 1)


@pytest.mark.parametrize("family,name", TIES, ids=_ids(TIES))
def test_tie_scenes_have_ties(family, name):
    """At least 10 records whose first calculateRayCollision call has two candidates at equal dst, and that dst the
    smallest: the choice between them is the record's winner.  The whole sphere tie scene is the exception its geometry
    forces: the triangle lies in front of the two equal spheres for every ray but the centre one, so there the 10 records
    have two candidates at equal dst behind the winner and one, the centre ray, has all three at the smallest (4.0f);
    tie_wide_spheres, the same spheres without the triangle, has the 10 at the smallest."""
    case = BY_NAME[family, name]
    rays, _, _ = rc.checked_inputs(family, case)
    cand = _first_call_candidates(case, rays)
    best = cand.min(1)
    closest = np.isfinite(best) & ((cand == best[:, None]).sum(1) >= 2)
    srt = np.sort(cand, 1)
    anywhere = (np.isfinite(srt[:, :-1]) & (srt[:, :-1] == srt[:, 1:])).any(1)
    print(f"{name}: of {len(rays)} records {int(closest.sum())} tie at the smallest dst of their first call, "
          f"{int(anywhere.sum())} at some dst")
    if name == "tie_wide":
        centre = case.pixels == case.width // 2 + case.height // 2 * case.width
        assert anywhere.sum() >= 10 and closest[centre].all() and centre.sum() == 1
        assert (cand[centre] == np.float32(4.0)).all()
    else:
        assert closest.sum() >= 10


def test_boxes_reach_max_bounce():
    """Records of exactly maxBounce calls for 63, 64, 65 and 100: such a path draws 7 values per call (RandomDiretion's
    six and the roulette's one), so the reference's seed_after is the seed advanced by 7 maxBounce draws."""
    import progressive_reference as pr

    for mb in (63, 64, 65, 100):
        full = 0
        for name, fx in rc.fixture("boxes").items():
            if fx.max_bounce != mb:
                continue
            seeds = fx.pixels.astype(np.uint32)
            full += int((pr.advance(seeds, 7 * mb) == fx.seed_after).sum())
        print(f"boxes maxBounce {mb}: {full} records of exactly {mb} calls")
        assert full >= 10, mb
