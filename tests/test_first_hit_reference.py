"""The premises of tests/test_gpu_first_hit.py, from the CPU oracle alone (tests/first_hit_reference.py), so that a case
that no longer covers its risk fails here, without a GPU: the golden scenes' launches have hits and misses, the tie cases
have their ties and the reference's winner, the NaN normals are somebody's closest hit, the closing sphere leaves no miss,
and the partitions' rows are the whole frame's.  Reference: calculateRayCollision (raytracing.c:216-240)."""
from __future__ import annotations

import numpy as np
import pytest

import adversarial_scenes as adv
import first_hit_reference as fr
from primary_rays import NO_HIT_DST, launch_rows


@pytest.mark.parametrize("shape", fr.SHAPES)
@pytest.mark.parametrize("name", fr.GOLDEN + fr.OUTSIDE)
def test_golden_launches_have_hits_and_misses(name, shape):
    """Hits and misses both occur -- except from the default scene's golden camera, which stands inside its closed box:
    there every ray hits, and the same scene seen from outside (fr.OUTSIDE) has the misses."""
    e = fr.expected(name, shape)
    hit = e["prim"] != -1
    if name in fr.CLOSED:
        assert hit.all() and (e["prim"] >= 0).any()
    else:
        assert hit.any() and (~hit).any(), f"{name} {shape}: {int(hit.sum())} hits of {hit.size}"
    assert (e["depth"][~hit] == NO_HIT_DST).all() and (e["depth"][hit] < NO_HIT_DST).all()
    assert not e["normal"][~hit].view(np.uint32).any() and not e["albedo"][~hit].view(np.uint32).any()
    if name.startswith("default_spheres"):
        assert (e["prim"] == -2).any() and (e["prim"] >= 0).any()
    if name == "suze":
        assert len(fr.geometry(name)[0]) > 64 and (e["prim"] >= 64).any(), "two mask words, the second one used"


@pytest.mark.parametrize("shape", fr.SHAPES)
def test_tie_scene_centre_pixel(shape):
    """The triangle and both spheres at distance exactly 4 along the centre ray: sphere 0 wins."""
    e = fr.expected("tie_scene", shape)
    cy, cx = shape[1] // 2, shape[0] // 2
    assert e["prim"][cy, cx] == -2 and e["depth"][cy, cx] == np.float32(4.0)
    assert (e["prim"] == 0).any() and not (e["prim"] == -3).any()


@pytest.mark.parametrize("name", ["ties_axis", "ties_tilted", "ties_rotated"])
def test_adversarial_ties_keep_the_lowest_index(name):
    """P0 (index 0) and P1 (index 9) overlap in one plane: where both are hit P0 wins, so P0 is seen over the whole overlap
    and P1 only beside it (ties_rotated: the same triangle twice, P1 never)."""
    e = fr.expected(name, fr.SHAPES[1])
    assert (e["prim"] == 0).sum() > 50
    if name == "ties_rotated":
        assert not (e["prim"] == 9).any()


def test_nan_normals_are_closest_hits():
    e = fr.expected("bad_normals", fr.SHAPES[1])
    tris = fr.geometry("bad_normals")[0]
    for t in adv.NAN_NORMALS["bad_normals"]:
        sel = e["prim"] == t
        assert sel.any(), f"triangle {t} (a NaN normal) is nobody's closest hit"
        want = tris.view(np.uint32).reshape(len(tris), 17)[t, 9:12]
        assert np.isnan(want.view(np.float32)).any()
        assert (e["normal"][sel].view(np.uint32) == want).all()


def test_sphere_cases():
    e = fr.expected("closing_sphere", fr.SHAPES[1])
    assert (e["prim"] == -2).all(), "every ray starts inside the sphere"
    e = fr.expected("open33", fr.SHAPES[1])
    assert (e["prim"] <= -2).any() and (e["prim"] >= 0).any()
    assert len(fr.geometry("open33")[1]) == 33


@pytest.mark.parametrize("shape", fr.SHAPES)
def test_partitions_are_the_whole_frames_rows(shape):
    """The expectation does not depend on the partition: rows (1, 3) and the two ranks of bands of 8."""
    whole = fr.expected("cube", shape)
    for kw in (dict(row_start=1, row_stride=3), dict(row_start=0, row_stride=2, row_band=8),
               dict(row_start=8, row_stride=2, row_band=8)):
        part = fr.expected("cube", shape, **kw)
        ys = launch_rows(fr.config("cube", shape, **kw))
        assert len(ys) > 0
        assert fr.differing(part, {k: v[ys] for k, v in whole.items()}) == dict.fromkeys(fr.NAMES, 0)
    ys = np.concatenate([launch_rows(fr.config("cube", shape, row_start=8 * r, row_stride=2, row_band=8)) for r in (0, 1)])
    assert sorted(ys) == list(range(shape[1]))
