"""tests/progressive_reference.py is right, and the scenes of tests/test_gpu_progressive.py are not vacuous (CPU only).

Right: chaining reference_pass over any split of a frame's samples reproduces oracle.render's accumulator, Color frame and
segment count bit for bit (the helper derives the segments from calc_color's states and a second, brighter sky).

Not vacuous: on the launch the GPU test renders (64x40, maxBounce 4) every scene has pixels whose state never moves (no hit
in any sample), pixels with exactly one hit in every sample, pixels with two or more hits in some sample, and -- after
every pass but the last -- pixels whose accumulator differs in bits from final * done / spp, so a kernel that rescaled
the finished frame instead of resuming would fail.  The counts are printed.  The reference's default box is closed: every
primary ray hits and every path bounces again, so it has no pixel of the first two kinds (asserted as such: it is what sends
the scene to the one-lane-per-pixel kernel); the other two counts must be positive there too."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import progressive_reference as pr
from raytracingc_amd._abi import RTC_F_DEBUG_BOUNCES, RtcRenderDesc

W, H, MAX_BOUNCE = 64, 40, 4
SPLITS = {12: ([12], [1] * 12, [5, 1, 6]), 70: ([70], [3, 64, 3])}
CLOSED = ("default",)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _desc(name, spp, mb=MAX_BOUNCE, flags=0, row_start=0, stride=1, band=0):
    return RtcRenderDesc(W, H, spp, mb, pr.geometry(name)[4], row_start, stride, flags, band)


@functools.lru_cache(maxsize=None)
def _cache(name):
    return {}


@pytest.mark.parametrize("spp", sorted(SPLITS))
@pytest.mark.parametrize("name", pr.SCENE_NAMES)
def test_chained_passes_reproduce_the_oracle(name, spp):
    tris, sph, scene, cam, _ = pr.geometry(name)
    d = _desc(name, spp)
    ocol, oacc, oseg = orc.render(tris, sph, scene, cam, d, threads=8)
    for split in SPLITS[spp]:
        ch = pr.chain(tris, sph, scene, cam, d, split, _cache(name))
        done, acc, rng, col, _ = ch[-1]
        assert done == spp
        assert int((_bits(acc) != _bits(oacc)).sum()) == 0, f"{name} {split}: accumulator bits"
        assert np.array_equal(col, ocol), f"{name} {split}: Color"
        assert sum(c[4] for c in ch) == oseg, f"{name} {split}: segments"


@pytest.mark.parametrize("case", ["mb0", "mb1", "debug", "rows_1_3", "bands_8_2"])
def test_other_launches_reproduce_the_oracle(case):
    """maxBounce 0 and 1, calcDebugColor and row / band shares (launch rows, not image rows, index the buffers)."""
    name = "ultracomplex"
    tris, sph, scene, cam, _ = pr.geometry(name)
    d = {"mb0": _desc(name, 12, mb=0), "mb1": _desc(name, 12, mb=1), "debug": _desc(name, 12, flags=RTC_F_DEBUG_BOUNCES),
         "rows_1_3": _desc(name, 12, row_start=1, stride=3), "bands_8_2": _desc(name, 12, stride=2, band=8)}[case]
    ocol, oacc, oseg = orc.render(tris, sph, scene, cam, d, threads=8)
    ch = pr.chain(tris, sph, scene, cam, d, [5, 1, 6])
    assert int((_bits(ch[-1][1]) != _bits(oacc)).sum()) == 0 and np.array_equal(ch[-1][3], ocol)
    assert sum(c[4] for c in ch) == oseg
    assert ch[-1][1].shape == oacc.shape


@pytest.mark.parametrize("spp", sorted(SPLITS))
@pytest.mark.parametrize("name", pr.SCENE_NAMES)
def test_scenes_are_not_vacuous(name, spp):
    tris, sph, scene, cam, _ = pr.geometry(name)
    d = _desc(name, spp)
    hits = pr.hits_per_sample(tris, sph, scene, cam, d, _cache(name))
    zero, one, multi = int((hits == 0).all(0).sum()), int((hits == 1).all(0).sum()), int((hits >= 2).any(0).sum())
    ch = pr.chain(tris, sph, scene, cam, d, SPLITS[spp][-1], _cache(name))
    final = ch[-1][1]
    not_rescaled = []
    for done, acc, rng, _, _ in ch[:-1]:
        scaled = (final * np.float32(done / spp)).astype(np.float32)
        not_rescaled.append(int((_bits(scaled) != _bits(acc)).any(-1).sum()))
        # the state is the seed 7 draws on per hit so far
        moved = int((rng.reshape(-1) != pr.seeds(d)).sum())
        assert moved == int((hits[:done] > 0).any(0).sum())
    print(f"{name} spp {spp}: {zero} pixels never hit, {one} with one hit in every sample, {multi} with >= 2 hits in some "
          f"sample, most hits {int(hits.max())}; pixels whose partial sum is not final * done / spp: {not_rescaled}")
    if name in CLOSED:
        assert zero == 0 and one == 0  # a closed scene: every sample bounces more than once
    else:
        assert zero > 0 and one > 0
    assert multi > 0
    assert not_rescaled and min(not_rescaled) > 0
