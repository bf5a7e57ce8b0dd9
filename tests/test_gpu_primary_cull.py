"""Soundness of the primary cull (the primary filter of rtc_prep_primary / prim_backfacing / prim_pass and the
tile prefilter rect_cone / tile_prunes at levels 0, 1 and 2) on the adversarial scenes (tests/adversarial_scenes.py).

rtc_probe_primary_cull runs a launch's own preparation and culls and returns the per-pixel filter's verdict for every
(pixel, triangle) pair -- evaluated by the render kernels' own functions on the launch's records -- with the tiles'
candidate bit-sets and pixel masks.  Whether a pair is a hit is decided here on the CPU by oracle.ray_triangle on the
float32 restatement of the pixel's primary ray (tests/primary_rays.py; tests/test_gpu_item_records.py pins the device's
rays to it bit for bit): a hit is a pair rayTriangle reports below calculateRayCollision's initial 999999.

For every launch: no hit is filtered out, per pixel, per tile or in the pixel mask, and a tile's bit-set is exactly the OR
of the per-pixel verdicts over its pixels, so the prefilter drops only what the per-pixel filter drops everywhere, and
nothing else."""
from __future__ import annotations

import numpy as np
import pytest

import oracle.binding as orc
import raytracingc_amd as rt
from adversarial_scenes import SCENES
from primary_rays import hit_table, launch_rays, prep_records, tile_cones

pytestmark = pytest.mark.gpu

SHAPES = {"64x40": dict(width=64, height=40), "33x17": dict(width=33, height=17)}


def _check(name, cfg, expect_level0=False):
    tris, cam, note = SCENES[name]
    T, W, rows = len(tris), cfg.width, cfg.rows()
    p = rt.primary_cull_probe(tris, rt.default_scene(), cam, cfg)
    assert p["level0"] == expect_level0
    tx = p["tiles_x"]
    assert tx == 2 * ((W + 15) // 16) and p["tiles"] == tx * 2 * ((rows + 15) // 16) and p["words"] == ((T + 7) // 8 * 8 + 63) // 64
    rec, _ = hit_table(orc.ray_triangle, tris, launch_rays(cam, cfg))
    kept = p["kept"].reshape(rows * W, T) != 0
    r, x = np.divmod(np.arange(rows * W), W)
    tile, bit = (r >> 3) * tx + (x >> 3), ((r & 7) << 3) | (x & 7)
    # the tiles' bit-sets as [tiles, 64 * words] booleans
    tb = ((p["tile_bits"][:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    tb = tb.reshape(p["tiles"], -1)
    pm = ((p["pix_mask"][tile] >> bit.astype(np.uint64)) & np.uint64(1)).astype(bool)
    what = f"{name} {W}x{cfg.height} rows {cfg.row_start}+{cfg.row_stride}/{cfg.row_band}"
    hits, nonhit = int(rec.sum()), int((~rec).sum())
    print(f"{what}: {hits} hits in {rec.size} pairs, kept {int(kept.sum())}, rejected non-hits {int((~kept & ~rec).sum())}, "
          f"tile bits {int(tb.sum())}, geometry pixels {int(pm.sum())}")
    lost = rec & ~kept
    assert not lost.any(), f"{what}: the filter rejects {int(lost.sum())} hits, first (pixel, triangle) {np.argwhere(lost)[0]}"
    lost = rec & ~tb[tile, :T]
    assert not lost.any(), f"{what}: {int(lost.sum())} hits are missing from their tile's bit-set, first {np.argwhere(lost)[0]}"
    lost = rec.any(1) & ~pm
    assert not lost.any(), f"{what}: {int(lost.sum())} pixels with a hit have their pixMask bit clear"
    # a tile's bit-set is the OR of the per-pixel verdicts over its valid pixels, in both directions
    want = np.zeros_like(tb)
    np.logical_or.at(want, (tile, slice(0, T)), kept)
    diff = want != tb
    assert not diff.any(), (f"{what}: {int((tb & ~want).sum())} bits set for triangles no pixel keeps, "
                            f"{int((want & ~tb).sum())} kept triangles pruned by the prefilter, first {np.argwhere(diff)[0]}")
    assert np.array_equal(pm, kept.any(1)), f"{what}: pixMask is not 'some triangle kept'"
    # non-vacuity
    if "filter active" in note:
        assert int((~kept & ~rec).sum()) * 2 >= nonhit, f"{what}: the filter rejects less than half of the non-hit pairs"
    # triangles the filter is disabled for (sane false; not `never`) are kept everywhere
    prep = prep_records(tris, cam.origin)
    off = np.flatnonzero(~prep["sane"] & ~prep["never"])
    assert kept[:, off].all(), f"{what}: a triangle whose filter is disabled is rejected somewhere"
    _check_constants(what, p, prep, cam, cfg, note, want, T)
    return p


def _close(got, want, rtol):
    """Equal, both NaN, or within rtol (infinities must match exactly)."""
    got, want = got.astype(np.float64), want.astype(np.float64)
    with np.errstate(all="ignore"):
        return (got == want) | (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= rtol * np.abs(want))


def _check_constants(what, p, prep, cam, cfg, note, kept_by_tile, T):
    """The margins the proofs derive, by value.  The hit-based assertions above cannot see a margin that is too small by
    less than the proofs' own slack (every per-triangle bound is taken 4x, the cone's direction bound carries 16 / 3 over
    the three roundings it covers): real rounding errors stay inside the remaining margin, so a dropped term or a halved
    eDir changes no verdict on any scene.  The records and the cones are therefore also compared with restatements of
    rtc_prep_primary and rect_cone in double (tests/primary_rays.py) that carry the constants of DESIGN 3.1: 9.006 u,
    6.002 u, 2.0002 u, 4.8e-7, 2.5e-4, 16 u S / vmin + 4 u.  One float32 ulp (2^-23) is allowed on the records: the margins
    are double expressions rounded outwards, and an evaluation-order difference in the last double bit may move that
    rounding by one step."""
    bad = ~_close(p["prim_f"], prep["rec"], 2.0 ** -23)
    assert not bad.any(), (f"{what}: DevPrimF differs from rtc_prep_primary's restatement at (triangle, field) "
                           f"{np.argwhere(bad)[:4].tolist()}: {p['prim_f'][bad][:4]} vs {prep['rec'][bad][:4]}")
    cones = tile_cones(cam, cfg, p["tiles_x"], p["tiles"])
    ok = p["cones"][:, 3] != 0
    assert np.array_equal(ok, cones[:, 3] != 0), f"{what}: the usable cones differ from rect_cone's restatement"
    bad = ~_close(p["cones"][ok, :3], cones[ok, :3], 1e-12)
    assert not bad.any(), f"{what}: eDir / vmin / vmax differ from rect_cone's restatement: {p['cones'][ok][bad.any(1)][:2]}"
    # the frame's own tiles (those with a valid pixel) are usable, except where the scene is built to disable the prefilter
    tx, rows = p["tiles_x"], cfg.rows()
    inside = np.array([(t % tx) * 8 < cfg.width and (t // tx) * 8 < rows for t in range(p["tiles"])])
    if "no tile is prefiltered" in note:
        assert not ok.any() and not p["pruned"].any(), f"{what}: a cone is usable"
    else:
        assert ok[inside].all(), f"{what}: a tile's cone is not usable"
    # the tile's own prefilter prunes only triangles no pixel of the tile keeps, and is not idle where the filter is active
    # (every such scene has triangles behind the camera or off to one side of the frame: some tile must prune some)
    pruned = p["pruned"] != 0
    assert not (pruned & kept_by_tile[:, :T]).any(), f"{what}: the prefilter prunes a triangle some pixel of the tile keeps"
    print(f"{what}: the tiles' prefilter prunes {int(pruned[inside].sum())} of {int((~kept_by_tile[inside, :T]).sum())} "
          f"(tile, triangle) pairs that no pixel keeps")
    if "filter active" in note and "no tile is prefiltered" not in note:
        assert pruned[inside].any(), f"{what}: the tiles' prefilter prunes nothing"


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_primary_cull_is_sound(name, shape, gpu_available):
    _check(name, rt.RenderConfig(spp=1, max_bounce=4, triangles_only=True, **SHAPES[shape]))


@pytest.mark.parametrize("row_start", [8, 16])
def test_primary_cull_row_partitioned(row_start, gpu_available):
    """Bands of 8 rows with stride 3: rect_cone maps launch rows to y (rows 16-23 hold the slivers' middle row)."""
    _check("slivers", rt.RenderConfig(64, 40, 1, 4, True, row_start=row_start, row_stride=3, row_band=8))


def test_primary_cull_with_the_superblock_level(gpu_available):
    """1024 x 448 = 458,752 pixels, above rtcplan::kSuperCullPixels (400,000): rtc_super_cull runs (level 0), on the
    smallest scene with slivers and a far-offset camera (24 triangles: 11 M pairs)."""
    p = _check("far_offset_1e3", rt.RenderConfig(1024, 448, 1, 4, True), expect_level0=True)
    assert p["level0"]
