"""tests/footprints.py on the CPU: the checker catches what it must on synthetic snapshots, and every case of the matrix
tests/test_gpu_footprints.py runs plans what it is meant to exercise (rtc_plan_sim_*: the planner the executor runs, no
GPU).  No reference counterpart: the scratch, its slots and the plan are this project's."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import footprints as fpt
import raytracingc_amd as rt
from conftest import REPO
from footprints import READ, WRITE, Sim
from raytracingc_amd import _abi

CASES = {c.name: c for c in fpt.LAUNCHES}


def _spans(scratch_bytes):
    """Synthetic spans in rtc_scene_spans' order: 4 KB each outside the scratch, the pool 64 blocks."""
    rows = [(fpt.RES_SCRATCH, 0, 0, scratch_bytes)]
    rows += [(fpt.RES_PRIM, h, part, 4096) for h in range(fpt.SLOTS) for part in (0, 1)]
    rows += [(fpt.RES_GEOSET, q, 0, 2048) for q in range(fpt.GEO_RING)]
    rows += [(fpt.RES_SAMPLES, 0, 0, 4096), (fpt.RES_SEGSLOTS, 0, 0, 4096)]
    rows += [(fpt.RES_SCENE_GEN, g, k, 4096) for g in range(2) for k in range(6)]
    rows += [(fpt.RES_DRAW_TABLE, 0, part, 4096) for part in range(3)]
    rows += [(fpt.RES_ITEM_DRAW, h, 0, 4096) for h in range(fpt.SLOTS)]
    rows += [(fpt.RES_MEMBERSHIP, 0, 0, 4096), (fpt.RES_DRAW_POOL, 0, 0, 64 * 1024)]
    assert len(rows) == fpt.SPAN_COUNT
    return np.array([(r, i, p, 0x10000 * (n + 1), b) for n, (r, i, p, b) in enumerate(rows)], np.uint64)


def _index(spans, res, ident=0, part=0):
    return next(i for i, s in enumerate(spans) if (int(s[0]), int(s[1]), int(s[2])) == (res, ident, part))


def _planned(name, launches_before=0):
    """(ops, rows, trailer, regions, scratch bytes) of a case planned on a fresh scene after `launches_before` of itself."""
    case = CASES[name]
    sim = Sim(case.scene, case.cache)
    try:
        for _ in range(launches_before + 1):
            ops, rows, trailer = sim.launch(case, case.camera_args()[0])
        out = (C.c_ulonglong * 48)()
        assert sim.L.rtc_plan_sim_regions(sim.h, out, 16) >= 2
        return ops, rows, trailer, sim.regions(), int(out[3])
    finally:
        sim.close()


def _snapshots(spans):
    before = [np.zeros(int(s[4]), np.uint8) for s in spans]
    return before, [b.copy() for b in before]


def _fill_allowed(after, allowed):
    for i, ranges in allowed.items():
        for lo, hi in ranges:
            after[i][lo:hi] = 0xff


def _covered(allowed, i, off):
    return any(lo <= off < hi for lo, hi in allowed.get(i, []))


def test_exactly_the_declared_ranges_pass_and_their_edges_do_not():
    ops, rows, _, regions, cap = _planned("split_deferred_cube")
    spans = _spans(cap)
    allowed = fpt.allowed_ranges(rows, spans)
    before, after = _snapshots(spans)
    _fill_allowed(after, allowed)
    assert sum(int((a != 0).sum()) for a in after) > 0
    assert fpt.violations(before, after, allowed) == []
    # one byte before a region and the byte at its end, wherever no other declared write lies there
    edges = 0
    for name, (lo, hi) in regions.items():
        for off in (lo - 1, hi):
            if off < 0 or _covered(allowed, 0, off) or not _covered(allowed, 0, lo):
                continue
            b, a = _snapshots(spans)
            a[0][off] = 1
            assert fpt.violations(b, a, allowed) == [(0, off)], (name, off)
            edges += 1
    assert edges >= 2


def test_another_slots_region_and_the_gaps_are_violations():
    ops, rows, _, regions, cap = _planned("merge_small_share", launches_before=2)  # slot 2
    spans = _spans(cap)
    allowed = fpt.allowed_ranges(rows, spans)
    stride = cap // fpt.SLOTS
    slot = regions["mask"][0] // stride
    assert slot == 2 and regions["mask"][0] == slot * stride
    for name in ("geoList", "pixItem", "geoColor"):
        lo, _ = regions[name]
        for other in (lo - stride, lo + stride):  # the same region of the slots beside it
            b, a = _snapshots(spans)
            a[0][other] = 1
            assert fpt.violations(b, a, allowed) == [(0, other)], (name, other)
    # the alignment gap before pixItem (256-byte aligned behind the superblock words' place) or, where the offsets happen
    # to be aligned, none: every byte of the slot outside its bound regions is a violation
    inside = np.zeros(stride, bool)
    for lo, hi in regions.values():
        inside[lo - slot * stride: hi - slot * stride] = True
    gaps = np.flatnonzero(~inside) + slot * stride
    assert len(gaps)
    for off in (int(gaps[0]), int(gaps[len(gaps) // 2]), int(gaps[-1])):
        b, a = _snapshots(spans)
        a[0][off] = 1
        assert fpt.violations(b, a, allowed) == [(0, off)]
    # the historical padding behind geoColor: an int per tile (rtc_plan.cpp layout_slot), inside the slot, in no region
    tiles = 4 * ((64 + 15) // 16) * ((40 + 15) // 16)
    pad = regions["geoColor"][1]
    assert pad + 4 * tiles <= (slot + 1) * stride and not inside[pad - slot * stride: pad - slot * stride + 4 * tiles].any()
    b, a = _snapshots(spans)
    a[0][pad: pad + 4 * tiles] = 7
    assert [o for _, o in fpt.violations(b, a, allowed)] == list(range(pad, pad + 4 * tiles))


def test_the_padding_behind_the_order_is_a_violation():
    """layout_slot keeps the sub-list counters' old place behind kBufOrder (16 x 32 ints): no kernel may write it."""
    ops, rows, _, regions, cap = _planned("no_coop")
    spans = _spans(cap)
    allowed = fpt.allowed_ranges(rows, spans)
    pad = regions["order"][1]
    assert all(not (lo < pad + 2048 and pad < hi) for lo, hi in regions.values())
    b, a = _snapshots(spans)
    a[0][pad] = a[0][pad + 2047] = 1
    assert fpt.violations(b, a, allowed) == [(0, pad), (0, pad + 2047)]
    b, a = _snapshots(spans)
    a[0][regions["order"][0]: pad] = 1
    assert fpt.violations(b, a, allowed) == []


def test_generations_counter_sets_and_the_pool():
    ops, rows, _, _, cap = _planned("cached_cold", launches_before=3)  # the fourth split launch: counter sets 3 and 4
    spans = _spans(cap)
    allowed = fpt.allowed_ranges(rows, spans, pool_taken=10)
    sets = sorted(int(spans[i][1]) for i in allowed if int(spans[i][0]) == fpt.RES_GEOSET)
    assert sets == [3, 4]
    for q in range(fpt.GEO_RING):
        b, a = _snapshots(spans)
        i = _index(spans, fpt.RES_GEOSET, q)
        a[i][100] = 1
        assert fpt.violations(b, a, allowed) == ([] if q in sets else [(i, 100)])
    for g in range(2):  # a launch writes neither generation
        for k in range(6):
            b, a = _snapshots(spans)
            i = _index(spans, fpt.RES_SCENE_GEN, g, k)
            a[i][0] = 1
            assert fpt.violations(b, a, allowed) == [(i, 0)]
    for res, ident in ((fpt.RES_PRIM, 1), (fpt.RES_ITEM_DRAW, 1), (fpt.RES_MEMBERSHIP, 0), (fpt.RES_SAMPLES, 0),
                       (fpt.RES_SEGSLOTS, 0)):  # another slot's records and arrays; what an in-kernel sum leaves alone
        b, a = _snapshots(spans)
        i = _index(spans, res, ident)
        a[i][8] = 1
        assert fpt.violations(b, a, allowed) == [(i, 8)]
    # the pool is append-only: the blocks taken before the launch stay, those behind them may be filled
    pool = _index(spans, fpt.RES_DRAW_POOL)
    b, a = _snapshots(spans)
    a[pool][10 * 1024 - 1] = a[pool][10 * 1024] = a[pool][-1] = 1
    assert fpt.violations(b, a, allowed) == [(pool, 10 * 1024 - 1)]
    # ... and a launch that takes no block writes none
    ops, rows, _, _, cap = _planned("chain_inline")
    allowed = fpt.allowed_ranges(rows, _spans(cap), pool_taken=0)
    b, a = _snapshots(_spans(cap))
    a[pool][5000] = 1
    assert fpt.violations(b, a, allowed) == [(pool, 5000)]


def test_an_update_writes_one_generation_and_a_regroup_the_membership_too():
    sim = Sim("cube")
    ops_a, fp_a = (C.c_int * 256)(), (C.c_ulonglong * (6 * 256))()
    try:
        rc = sim.L.rtc_plan_sim_update(sim.h, 0, ops_a, 64, fp_a, 256)
        ops, rows, trailer = fpt.split_plan(np.frombuffer(ops_a, np.int32, 4 * (rc & 0xff)).copy(),
                                            np.frombuffer(fp_a, np.uint64, 6 * (rc >> 8)).copy())
        assert int(trailer[2]) == 1 and fpt.named_rows(ops, rows) == {("refit", "scene_gen", WRITE), ("refit", "scene_gen", READ)}
        spans = _spans(4096)
        allowed = fpt.allowed_ranges(rows, spans)
        b, a = _snapshots(spans)
        _fill_allowed(a, allowed)
        assert fpt.violations(b, a, allowed) == []
        assert {(int(spans[i][0]), int(spans[i][1])) for i in allowed} == {(fpt.RES_SCENE_GEN, 1)}
        i = _index(spans, fpt.RES_SCENE_GEN, 0, 3)
        a[i][17] = 1
        m = _index(spans, fpt.RES_MEMBERSHIP)
        a[m][0] = 1
        assert fpt.violations(b, a, allowed) == [(i, 17), (m, 0)]
        rc = sim.L.rtc_plan_sim_regroup(sim.h, 0, 0x9000, ops_a, 64, fp_a, 256)
        ops, rows, trailer = fpt.split_plan(np.frombuffer(ops_a, np.int32, 4 * (rc & 0xff)).copy(),
                                            np.frombuffer(fp_a, np.uint64, 6 * (rc >> 8)).copy())
        named = fpt.named_rows(ops, rows)
        assert ("regroup_index", "membership", WRITE) in named and ("regroup_centroids", "regroup_scratch", WRITE) in named
        allowed = fpt.allowed_ranges(rows, spans)
        assert {(int(spans[i][0]), int(spans[i][1])) for i in allowed} == {(fpt.RES_SCENE_GEN, 0), (fpt.RES_MEMBERSHIP, 0)}
    finally:
        sim.close()


def test_the_queries_declare_no_write_of_the_scenes():
    """rtc.h: a query uses no scratch, primary record, counter set, stream or event of the scene's."""
    sim = Sim("cube")
    L, o, f = sim.L, (C.c_int * 256)(), (C.c_ulonglong * (6 * 256))()
    hit = (C.c_ulonglong * 4)(0x100, 0x200, 0, 0)
    wave = rt.RTC_F_WAVE_PER_RAY
    queries = [("trace_rays", lambda: L.rtc_plan_sim_trace_rays(sim.h, 0, 0x10, hit, 0, o, 64, f, 256)),
               ("trace_paths", lambda: L.rtc_plan_sim_trace_paths(sim.h, 0, 0x10, 0x20, 0x30, 0x40, 1, 0, 0, o, 64, f, 256)),
               ("trace_paths", lambda: L.rtc_plan_sim_trace_paths(sim.h, 0, 0x10, 0x20, 0x30, 0, 0, 2, wave, o, 64, f, 256)),
               ("occluded", lambda: L.rtc_plan_sim_occluded(sim.h, 0, 0x10, 0x20, 0x30, 1, 0, o, 64, f, 256)),
               ("render_pixels", lambda: L.rtc_plan_sim_render_pixels(sim.h, 0, 0x10, 0x20, 0x30, 0x40, 0, 0, 0, o, 64, f, 256)),
               ("render_pixels", lambda: L.rtc_plan_sim_render_pixels(sim.h, 0, 0x10, 0x20, 0x30, 0x40, 1, 2, wave, o, 64, f,
                                                                      256))]
    try:
        for kernel, call in queries:
            rc = call()
            assert rc > 0 and rc & 0xff == 1
            ops, rows, _ = fpt.split_plan(np.frombuffer(o, np.int32, 4 * (rc & 0xff)).copy(),
                                          np.frombuffer(f, np.uint64, 6 * (rc >> 8)).copy())
            assert fpt.kernels_of(ops) == [kernel]
            named = fpt.named_rows(ops, rows)
            assert (kernel, "scene_gen", READ) in named and any(a in fpt.WRITES for _, _, a in named)
            assert not any(a in fpt.WRITES and n in fpt.SCENE_RES.values() for _, n, a in named), sorted(named)
            assert fpt.allowed_ranges(rows, _spans(4096), pool_taken=0) == {}
    finally:
        sim.close()


@pytest.mark.parametrize("name", [c.name for c in fpt.LAUNCHES if not c.name.startswith("overlap_")])
def test_a_case_plans_what_it_is_meant_to_exercise(name):
    case = CASES[name]
    sim = Sim(case.scene, case.cache)
    try:
        if case.prepare or case.name == "merge_small_share":
            sim.launch(case, case.camera_args()[1])
        if case.quiet:  # (as on the device: behind a joined launch from the same camera origin)
            sim.launch(CASES["chain_inline"], case.camera_args()[1])
        ops, rows, trailer = sim.launch(case, case.camera_args()[0])
        regions = sim.regions()
    finally:
        sim.close()
    named = fpt.named_rows(ops, rows, regions)
    for row in case.rows:
        assert row in named, (row, sorted(named))
    assert not set(case.absent) & set(fpt.kernels_of(ops)), fpt.kernels_of(ops)
    # the k-th scratch write row of a kernel is the region SCRATCH_WRITES names
    for region, lo, hi in fpt.scratch_write_rows(ops, rows):
        assert regions[region] == (lo, hi), (region, lo, hi, regions)
    # whatever must show a change is declared written
    declared = {n for _, n, a in named if a in fpt.WRITES} | ({"draw_pool"} if ("tile_cull", "draw_table", WRITE) in named else set())
    assert set(case.must) <= declared, set(case.must) - declared
    if case.quiet:
        assert not any(a in fpt.WRITES and n in fpt.SCENE_RES.values() for _, n, a in named), sorted(named)


def test_the_cases_take_the_routes_their_names_say():
    def plan(name, **kw):
        return _planned(name, **kw)

    assert "accum" in fpt.kernels_of(plan("split_deferred_cube")[0]) and "accum" not in fpt.kernels_of(plan("chain_inline")[0])
    assert fpt.kernels_of(plan("no_coop")[0])[-2:] == ["order", "render"]
    assert fpt.kernels_of(plan("default_sphere_one_lane")[0])[-2:] == ["order", "render"]
    assert fpt.kernels_of(plan("no_tile_cull")[0]) == ["prep", "render"]
    assert "reduce" in fpt.kernels_of(plan("segments")[0])
    assert "chain" in fpt.kernels_of(plan("open5_split_spheres")[0])
    for name in ("super_cull", "wide_items"):
        assert "super_cull" in fpt.kernels_of(plan(name)[0])
    kernels = fpt.kernels_of(plan("merge_small_share")[0])
    assert kernels.index("sky") > kernels.index("chain")  # merge: the sky pass behind the geometry kernel
    assert fpt.kernels_of(plan("first_hit_no_tile_cull")[0]) == ["prep", "first_hit"]
    assert fpt.kernels_of(plan("first_hit")[0]) == ["prep", "tile_cull", "first_hit"]


def test_nine_overlapped_launches_use_every_slot_and_both_cull_streams():
    sim = Sim("cube")
    slots, streams, written = [], set(), set()
    try:
        for k, case in enumerate(fpt.OVERLAPPED):
            ops, rows, trailer = sim.launch(case, case.camera_args()[k % 3])
            assert int(trailer[4]) == 1, "overlapped"
            slots.append(int(trailer[2]))
            streams |= {int(o[1]) for o in ops if int(o[0]) == 0}
            regions = sim.regions()
            for region, lo, hi in fpt.scratch_write_rows(ops, rows):
                assert regions[region] == (lo, hi)
                written.add(region)
            for row in case.rows:
                assert row in fpt.named_rows(ops, rows, regions)
    finally:
        sim.close()
    assert slots == [0, 1, 2, 3, 4, 5, 6, 7, 0] and streams == {0, 1, 2, 3}
    assert {"pixItem", "geoColor"} <= written


def test_the_matrix_declares_every_region_and_resource_written():
    declared = {"scene_gen", "membership"}  # (the update and the regroup: test_an_update_writes_one_generation...)
    for case in fpt.LAUNCHES:
        if case.name.startswith("overlap_"):
            continue
        declared |= set(case.must)
    assert declared >= fpt.WHOLE_MATRIX, fpt.WHOLE_MATRIX - declared


def test_every_allocation_of_a_scene_has_its_span():
    """rtc_scene_spans lists what rtc_scene.hip and rtc_render.hip's grow_capacity allocate: every hipMalloc of theirs is
    named here with the resource its span carries, so a new one fails until it has a span (and a row in this table)."""
    spans_of = {"D.table": 12, "D.ctr": 12, "D.blockSeed": 12, "D.pool": 21, "D.itemDraw": 13, "dev": 9, "s->clIndex": 18,
                "s->primF": 1, "s->primX": 1, "s->segSlots": 4, "s->geoCounts": 2, "buf": (0, 3)}
    src = os.path.join(REPO, "raytracingc_amd", "csrc")
    found = set()
    for unit in ("rtc_scene.hip", "rtc_render.hip"):
        found |= set(re.findall(r"hipMalloc\(&([\w.>-]+)", open(os.path.join(src, unit)).read()))
    assert found == set(spans_of)
    body = re.search(r'extern "C" int rtc_scene_spans\(.*?\n}\n', open(os.path.join(src, "rtc_scene.hip")).read(), flags=re.S).group(0)
    listed = re.findall(r"span\(rtcplan::kRes(\w+),", body)
    assert listed == ["Scratch", "Prim", "Prim", "GeoSet", "Samples", "SegSlots", "SceneGen", "DrawTable", "DrawTable",
                      "DrawTable", "ItemDraw", "Membership", "DrawPool"]
    render = open(os.path.join(src, "rtc_render.hip")).read()
    assert re.findall(r"regrow\(ms->(\w+),", render) == ["scratch", "samples"]


def test_the_hooks_refuse_null_arguments():
    L = rt.lib()
    ops, rows, out = (C.c_int * 192)(), (C.c_ulonglong * 1536)(), (_abi.RtcSpan * 64)()
    assert L.rtc_scene_last_plan(None, ops, 48, rows, 256) == _abi.RTC_EINVAL and b"rtc_scene_last_plan" in L.rtc_last_error()
    assert L.rtc_scene_spans(None, out, 64) == _abi.RTC_EINVAL and b"rtc_scene_spans" in L.rtc_last_error()
    assert C.sizeof(_abi.RtcSpan) == 40 and hasattr(rt.DeviceScene, "last_plan") and hasattr(rt.DeviceScene, "spans")
