"""What tests/large_scenes.py claims about its scenes, from the CPU oracle and the host records alone (no GPU); and the
tile cull's cap in the launch planner, through its CPU hooks.  tests/test_gpu_large_scenes.py runs the device on the same
data: a claim that fails here means that file checks less than it says.

Two orders index a scene.  The reference order is the caller's: triangle i of Triangle[].  The `tris` records of
rt.scene_records_host keep it (record i holds triangle i's vertices), rtc_prep_primary writes the primary filter's records
from them, and so bit b of word w of a tile's candidate mask is reference triangle 64 w + b: the MASK WORDS INDEX THE
REFERENCE ORDER.  The cluster order is the upload's: the clTris records (dword 12: the reference index, -1 for padding),
eight to a cluster, 32 clusters to a chunk; the bounce rays' chunk and cluster loops walk it.  Every claim about words is
stated in the reference order and every claim about chunks in the cluster order.

Counts measured (pixels hit / pixels; winners below word 256, from it on, in the last sixteenth of the words; in chunk 0,
in chunks >= 64, in the last sixteenth of the chunks; then the replay set's hits, misses and chunks):
  w257      1286 / 1920;  1164, 122, 186;  19, 122, 138;  1491 hit, 1257 miss, 64 chunks
  cap        523 /  561;    19, 504,  31;   1, 501,  36;   316 hit,  295 miss, 259 chunks
  past_cap   523 /  561;    19, 504,  31;   1, 501,  36;   316 hit,  296 miss, 256 chunks
At w257 the last word and the last chunk hold one triangle, the awning: 122 pixels see it, 27 replay rays hit it, and 31
pixels of the frame that do not see it change when it is taken away (their bounce rays reach it)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import footprints as fpt
import large_scenes as ls
import oracle.binding as orc
import raytracingc_amd as rt

NAMES = sorted(ls.CLASSES)


def _winners(name, which):
    prim = ls.expected(name, which)["prim"]
    return prim[prim >= 0].astype(np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_the_size_classes_are_what_the_table_says(name):
    T = ls.CLASSES[name]
    want = {"w257": (257, 2049, 65), "cap": (6144, 49152, 1536), "past_cap": (6145, 49153, 1537)}[name]
    assert ls.counts(T)[1:] == want and len(ls.tris(name)) == T
    # one triangle less does not cross the class's boundary
    assert ls.counts(16384)[1:] == (256, 2048, 64) and ls.counts(393216 - 8)[1] == 6144


@pytest.mark.parametrize("name", NAMES)
def test_upload_bookkeeping(name):
    """scene_records_host gives the table's cluster and chunk counts, the `tris` records keep the reference order, and the
    clustered records hold every triangle once; past_cap's padded count gives 6,145 words."""
    T = ls.CLASSES[name]
    rec, tris = ls.records(name), ls.tris(name)
    padded, words, clusters, chunks = ls.counts(T)
    assert len(rec["clTris"]) == padded and len(rec["clusters"]) == clusters and len(rec["chunks"]) == chunks
    assert (padded + 63) // 64 == words
    if name == "past_cap":
        assert padded == 393224 and words == 6145
    a = np.stack([tris["posA"][c] for c in "xyz"], 1)
    assert np.array_equal(rec["tris"][:T, :3].view(np.float32), a), "the tris records are in the reference order"
    ref = rec["clTris"][:, 12].view(np.int32)
    assert np.array_equal(np.sort(ref[ref >= 0]), np.arange(T)) and int((ref < 0).sum()) == padded - T
    assert not np.array_equal(ref[:T], np.arange(T)), "the cluster build has to regroup"
    if T % 8 == 1:  # the last cluster, and with it the last chunk, is the awning alone
        assert ref[-8] == T - 1 and (ref[-7:] == -1).all()
    assert ls.cluster_slot(name)[T - 1] // (ls.CLUSTER * ls.CHUNK) == chunks - 1


@pytest.mark.parametrize("name", NAMES)
def test_materials_differ_between_all_triangles(name):
    m = np.ascontiguousarray(ls.tris(name)["mat"]).view(np.uint32).reshape(-1, 5)
    assert len(np.unique(m, axis=0)) == len(m)
    mat = ls.tris(name)["mat"]
    assert 0 <= mat["smoothness"].min() and mat["smoothness"].max() <= 1 and mat["emissionStrength"].max() <= 1


@pytest.mark.parametrize("name", NAMES)
def test_primary_rays_reach_both_ends_of_both_orders(name):
    T = ls.CLASSES[name]
    _, words, _, chunks = ls.counts(T)
    pixels = ls.FRAME[name][0] * ls.FRAME[name][1]
    w = _winners(name, "frame")
    word, chunk = w // 64, ls.cluster_slot(name)[w] // (ls.CLUSTER * ls.CHUNK)
    got = dict(hit=len(w), low=int((word < 256).sum()), high=int((word >= 256).sum()),
               last_words=int((word >= words - words // 16).sum()), chunk0=int((chunk == 0).sum()),
               chunk64=int((chunk >= 64).sum()), last_chunks=int((chunk >= chunks - chunks // 16).sum()))
    print(name, pixels, got)
    assert 3 * got["hit"] >= pixels
    assert got["low"] and got["high"] and got["last_words"]
    assert got["chunk0"] and got["chunk64"] and got["last_chunks"]


@pytest.mark.parametrize("name", NAMES)
def test_the_replay_set_hits_and_misses(name):
    calls = ls.replay_calls(name)
    hit = calls["winner"] >= 0
    w = calls["winner"][hit].astype(np.int64)
    chunk = ls.cluster_slot(name)[w] // (ls.CLUSTER * ls.CHUNK)
    print(name, "replay", len(calls), "hit", int(hit.sum()), "miss", int((~hit).sum()), "chunks", len(np.unique(chunk)))
    assert hit.sum() >= 200 and (~hit).sum() >= 200
    assert len(np.unique(chunk)) >= 8
    # the replay rays times 3 leave the cluster bound: |dir|_1 beyond kClusterRhoMax
    d = np.abs(calls["dir"].astype(np.float64) * ls.RHO_SCALE).sum(1)
    assert (d > 4.0).sum() >= 200


def test_w257_bounce_rays_reach_the_one_triangle_of_the_last_word_and_chunk():
    """A dropped word 256 or chunk 64 must show in frames and queries alike: the awning, their one triangle, is seen by
    primary rays, hit by recorded bounce rays, and changes pixels of the frame that do not see it."""
    name, T = "w257", ls.CLASSES["w257"]
    assert T - 1 == 256 * 64 and ls.cluster_slot(name)[T - 1] == 64 * ls.CLUSTER * ls.CHUNK
    seen = (ls.expected(name, "frame")["prim"] == T - 1).reshape(ls.FRAME[name][1], ls.FRAME[name][0])
    replayed = int((ls.replay_calls(name)["winner"] == T - 1).sum())
    d = ls.frame_config(name).desc()
    without = orc.render(ls.tris(name)[:-1], None, rt.default_scene(), ls.frame_camera(name), d, threads=16)[1]
    changed = (without.view(np.uint32) != ls.frame_oracle(name)[1].view(np.uint32)).any(-1)
    print("w257 awning: pixels that see it", int(seen.sum()), "replay hits", replayed, "other pixels it changes",
          int((changed & ~seen).sum()))
    assert seen.sum() >= 20 and replayed >= 10 and (changed & ~seen).sum() >= 10


def test_the_query_rays_are_a_fixed_permutation_of_the_three_sets():
    for name in NAMES:
        rays, calls = ls.query_rays(name), ls.replay_calls(name)
        assert len(rays) == len(ls.launch_primary(name, "query")) + 2 * len(calls)
        assert not rays.flags.writeable and ls.query_rays(name) is rays


# ---- the tile cull's cap in the launch planner (rtc_plan.h kMaxCullMaskWords), through the rtc_plan_sim_* hooks --------------
def _plan(tri_count, size, **cfg):
    """(kernels, rtc_plan_sim_regions' rows) of one launch of `size` on a scene of tri_count triangles."""
    case = fpt.Case("plan", "w257", size=size, spp=1, cfg=tuple(cfg.items()))  # (the scene names the config, not the count)
    sim = fpt.Sim(case.scene, tri_count=tri_count)
    try:
        ops, rows, trailer = sim.launch(case, ls.camera_args(tri_count, *size))
        out = (C.c_ulonglong * (3 * 16))()
        n = sim.L.rtc_plan_sim_regions(sim.h, out, 16)
        return fpt.kernels_of(ops), [tuple(int(v) for v in out[3 * r:3 * r + 3]) for r in range(n)]
    finally:
        sim.close()


def test_the_same_request_plans_the_cull_at_the_cap_and_not_past_it():
    at, _ = _plan(ls.CLASSES["cap"], (33, 17))
    past, _ = _plan(ls.CLASSES["past_cap"], (33, 17))
    assert "tile_cull" in at and "chain" in at and "sky" in at
    assert "tile_cull" not in past and "chain" not in past and past == ["prep", "render"]
    # one triangle below the cap's last word, and the first-hit launch, decide alike
    assert "tile_cull" in _plan(ls.CLASSES["cap"] - 63, (33, 17))[0]
    assert "tile_cull" in _plan(ls.CLASSES["cap"], (33, 17), coop=False)[0]
    assert "tile_cull" not in _plan(ls.CLASSES["past_cap"], (33, 17), coop=False)[0]


def _slot_table(width, rows, words):
    """layout_slot (rtc_plan.cpp) in Python integers: ({region: (offset, bytes)}, slot bytes)."""
    gx, gy = (width + 15) // 16, (rows + 15) // 16
    blocks = gx * gy
    tiles = 4 * blocks
    sx, sy = (gx + 3) // 4, (gy + 3) // 4
    geo_cap = (tiles + 15) // 16 * 64
    entries, counters = 16 * geo_cap, 16 * 32 * 4
    table = [("mask", tiles * words * 8, 1, 0), ("pixMask", tiles * 8, 1, 0), ("weight", blocks * 4, 1, 0),
             ("order", (blocks + 4) * 4, 1, counters), ("geoList", entries * 16, 16, 0),
             ("superMask", sx * sy * words * 8, 8, 0), ("pixItem", tiles * 64 * 4, 256, 0),
             ("geoColor", entries * 4, 1, tiles * 4)]
    assert [t[0] for t in table] == fpt.REGIONS
    off = budget = 0
    out = {}
    for name, used, align, pad in table:
        start = (off + align - 1) // align * align
        out[name] = (start, used)
        off = start + used + pad
        budget += used + pad + (align if align > 1 else 0)
    return out, (budget + 255) // 256 * 256


def test_a_4k_launch_at_the_cap_lays_out_a_slot_past_32_bits():
    """3840 x 2160 at 6,144 words: the mask region alone is 129,600 tiles x 6,144 words x 8 bytes = 6.37e9 bytes.  The
    planner's offsets, sizes and slot size equal the region table in Python integers; nothing is allocated."""
    W, H, words = 3840, 2160, 6144
    kernels, regions = _plan(ls.CLASSES["cap"], (W, H))
    assert "super_cull" in kernels and "tile_cull" in kernels and "chain" in kernels
    want, slot = _slot_table(W, H, words)
    assert want["mask"][1] == 129600 * 6144 * 8 > 2 ** 32
    (slot_off, slot_bytes, need), (cap, _, bound) = regions[0], regions[1]
    assert (slot_off, slot_bytes, need, cap) == (0, slot, 8 * slot, 8 * slot)
    got = {fpt.REGIONS[r]: (off, size) for r, off, size in regions[2:]}
    # (the bound mask's low bits are the scratch regions, rtc_plan.h Buf; the bits above them are the caller's buffers)
    assert {"mask", "pixMask", "geoList", "superMask"} <= set(got)
    assert bound & (2 ** len(fpt.REGIONS) - 1) == sum(1 << fpt.REGIONS.index(k) for k in got)
    for name, where in got.items():
        assert where == want[name], (name, where, want[name])
    assert max(off + size for off, size in got.values()) <= slot
    # one word more: no cull, no slot
    kernels, regions = _plan(ls.CLASSES["past_cap"], (W, H))
    assert "tile_cull" not in kernels and regions[0] == (0, 0, 0) and len(regions) == 2
