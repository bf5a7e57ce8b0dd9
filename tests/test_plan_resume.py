"""The planner's side of the progressive passes (rtc_render_samples_async), on the CPU through rtc_plan_sim_*:
a pass binds the caller's RNG-state buffer and declares what its pixel kernels do with it and with the accumulator -- writes
in the frame's first pass, reads too in every later one --, is never overlapped, keeps to the caller's stream, and leaves
the planning of every other launch as it was.  The ordering checker is tests/test_plan.py's, unchanged."""
from __future__ import annotations

import ctypes as C

import pytest

import raytracingc_amd as rt
from test_plan import (ATOMIC, CAMS, ENVS, KERNEL, KEYED_WRITE, KNAMES, OVERLAP, READ, WRITE, Scenario, _check_bound_regions,
                       _desc)

RES_ACCUM, RES_RNG = 6, 8  # rtc_plan.h Res
STREAM, COLORS, ACCUM, RNG = 0x7f001000, 0x1000, 0xA000, 0xB000
PIXEL_KERNELS = {"sky", "chain", "accum", "render"}
# launches whose pixel kernels differ: the split launch with deferred sums and with in-kernel sums, a small share, the
# one-lane-per-pixel kernel behind the tile cull, calcDebugColor, and brute force (no scratch at all)
SHAPES = {
    "split_deferred": (_desc(1920, 1080, 64, 0, 1, 0, 0), {"sky", "chain", "accum"}),
    "split_inline": (_desc(640, 360, 16, 0, 1, 0, rt.RTC_F_CHAIN_INLINE), {"sky", "chain"}),
    "share": (_desc(1920, 1080, 64, 1, 4, 0, 0), {"sky", "chain"}),
    "no_coop": (_desc(640, 360, 16, 0, 1, 0, rt.RTC_F_NO_COOP), {"render"}),
    "debug": (_desc(640, 360, 16, 0, 1, 0, rt.RTC_F_DEBUG_BOUNCES), {"render"}),
    "brute": (_desc(256, 256, 16, 0, 1, 0, rt.RTC_F_NO_TILE_CULL), {"render"}),
}


def _pass(sc, d, first, count, segments=False, stream=STREAM, colors=COLORS, accum=ACCUM, rng=RNG, cam=CAMS[0]):
    assert sc.L.rtc_plan_sim_set_sample_range(sc.h, first, count, rng) == 0
    return sc.launch(d, stream, colors, accum, segments, cam, ENVS[0])


def _last_accesses(sc):
    """{kernel name: {(resource, access)}} of the last launch's accumulator and state rows."""
    out = {}
    for o, res, acc, ident, lo, hi, key, launch, k in sc.accesses:
        if launch == sc.n - 1:
            out.setdefault(KNAMES[k], set())
            if res in (RES_ACCUM, RES_RNG):
                assert ident == (ACCUM if res == RES_ACCUM else RNG)
                out[KNAMES[k]].add((res, acc))
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_first_pass_writes_and_later_passes_also_read(shape):
    d, kernels = SHAPES[shape]
    sc = Scenario(120)
    try:
        for first, count in ((0, 3), (3, d.spp - 4), (d.spp - 1, 1)):
            info = _pass(sc, d, first, count, segments=first == 3)
            assert not info["overlap"] and not info["alt"] and info["slot"] == 0
            assert {st for _, st in sc.kernel_order()} == {"caller"}  # no cull stream, no side stream: nothing unjoined
            acc = _last_accesses(sc)
            assert {k for k in acc if k in PIXEL_KERNELS} == kernels, acc
            for k in kernels:
                writes = {(RES_ACCUM, KEYED_WRITE), (RES_RNG, KEYED_WRITE)}
                reads = {(RES_ACCUM, READ), (RES_RNG, READ)}
                assert acc[k] == (writes if first == 0 else writes | reads), (shape, first, k, acc[k])
            for k in set(acc) - PIXEL_KERNELS:  # prep, culls, order, reduce: no pixel state
                assert acc[k] == set(), (k, acc[k])
            if d.flags & rt.RTC_F_NO_TILE_CULL == 0:
                _check_bound_regions(sc)
        assert sc.hazards() == []
    finally:
        sc.close()


def test_an_ordinary_launch_declares_no_state_and_no_reads():
    sc = Scenario(120)
    try:
        sc.launch(SHAPES["split_deferred"][0], STREAM, COLORS, ACCUM, False, CAMS[0], ENVS[0])
        acc = _last_accesses(sc)
        assert all(a == KEYED_WRITE and res == RES_ACCUM for rows in acc.values() for res, a in rows), acc
    finally:
        sc.close()


@pytest.mark.parametrize("legacy", [False, True])
def test_passes_interleaved_with_ordinary_launches_are_race_free(legacy):
    """Two progressive frames (one of a share, one whole) whose passes alternate with pipelined and joined launches of
    other buffers and cameras -- and one pipelined launch into the progressive frame's own Color buffer -- on two caller
    streams.  One frame size, so that the legacy slot layout (a test hook of tests/test_plan.py) is sound here too."""
    sc = Scenario(300, legacy=legacy)
    try:
        d = _desc(1920, 1080, 64, 0, 1, 0, 0)
        other = _desc(1920, 1080, 64, 0, 1, 0, OVERLAP)
        done = 0
        for k, count in enumerate([1, 15, 16, 31, 1]):
            _pass(sc, d, done, count, segments=k == 2)
            done += count
            for j in range(3):
                sc.launch(other, STREAM, 0x2000 + 0x1000 * j, 0, False, CAMS[(k + j) % 3], ENVS[j % 2])
            if k == 1:
                sc.launch(other, STREAM, COLORS, ACCUM, False, CAMS[1], ENVS[0])  # (it would ruin the frame; no race)
            if k == 3:
                sc.launch(_desc(1920, 1080, 16, 0, 1, 0, rt.RTC_F_HOIST_PRIMARY), 0, 0x2000, 0x9000, True, CAMS[2], ENVS[1])
            _pass(sc, d, 8 * k, 8, stream=0 if k % 2 else STREAM, colors=0x7000, accum=0x7100, rng=0x7200, cam=CAMS[1])
        assert done == 64
        assert sc.hazards() == []
    finally:
        sc.close()


def test_checker_sees_an_unordered_pass():
    """Not vacuous: with the waits dropped, a pass's reads race the unjoined sky pass of the pipelined launch before it."""
    sc = Scenario(120)
    try:
        d = _desc(1920, 1080, 64, 0, 1, 0, 0)
        _pass(sc, d, 0, 16)
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, COLORS, ACCUM, False, CAMS[0], ENVS[0])
        sc.model.wait = lambda st, ev: None
        _pass(sc, d, 16, 16)
        hz = [h for h in sc.hazards(limit=1000) if h[0] != "rng_state"]  # (on the buffers a launch has too)
        assert hz, "a pass that does not wait for the pending sky pass must race it"
    finally:
        sc.close()


@pytest.mark.parametrize("bad", ["overlap", "first<0", "count=0", "past_spp", "no_accum", "no_state"])
def test_refused_ranges(bad):
    L = rt.lib()
    sc = Scenario(120)
    try:
        d = _desc(640, 360, 16, 0, 1, 0, OVERLAP if bad == "overlap" else 0)
        first, count = {"first<0": (-1, 4), "count=0": (4, 0), "past_spp": (9, 8)}.get(bad, (4, 4))
        assert L.rtc_plan_sim_set_sample_range(sc.h, first, count, 0 if bad == "no_state" else RNG) == 0
        cam, env = (C.c_float * 13)(*CAMS[0]), (C.c_float * 14)(*ENVS[0])
        rc = L.rtc_plan_sim_launch(sc.h, C.byref(d), STREAM, COLORS, 0 if bad == "no_accum" else ACCUM, 0, cam, env, sc.ops,
                                   64, sc.fp, 256)
        assert rc == rt.RTC_EINVAL
        # the range applied to that launch alone, and a refused launch changed nothing: the next one is the first
        # ordinary launch of a fresh scene
        fresh = Scenario(120)
        try:
            sc.launch(d, STREAM, COLORS, ACCUM, False, CAMS[0], ENVS[0])
            fresh.launch(d, STREAM, COLORS, ACCUM, False, CAMS[0], ENVS[0])
            assert sc.last_ops == fresh.last_ops
            assert RES_RNG not in {a[1] for a in sc.accesses}
        finally:
            fresh.close()
    finally:
        sc.close()


def _rows(sc):
    """The last launch's footprint rows without the vector clocks: (kernel, resource, access, id, lo, hi)."""
    return sorted((KNAMES[a[8]], a[1], a[2], a[3], a[4], a[5]) for a in sc.accesses if a[7] == sc.n - 1)


def test_launches_without_a_range_plan_as_before():
    """A scene that renders passes between its ordinary launches plans those launches op for op, footprint row for
    footprint row, as a scene that never had a range set and ran the passes' launches joined and whole."""
    a, b = Scenario(300), Scenario(300)
    try:
        whole = _desc(1920, 1080, 64, 0, 1, 0, 0)
        seq = [(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), 0x2000, 0, False, 0), (whole, COLORS, ACCUM, False, 0),
               (_desc(1920, 1080, 64, 2, 8, 0, OVERLAP), 0x3000, 0, False, 1), (whole, COLORS, ACCUM, True, 0),
               (_desc(640, 360, 16, 0, 1, 0, rt.RTC_F_NO_COOP), 0x4000, 0x4100, False, 0),
               (_desc(3840, 2160, 16, 0, 1, 0, OVERLAP), 0x5000, 0, False, 2), (whole, COLORS, ACCUM, False, 0),
               (_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), 0x2000, 0, False, 0)]
        done = 0
        for d, colors, accum, seg, cam in seq:
            if accum == ACCUM:  # a's pass is b's ordinary joined launch of the same frame
                _pass(a, d, done, 16, segments=seg)
                done += 16
                b.launch(d, STREAM, colors, accum, seg, CAMS[cam], ENVS[0])
                continue
            ia = a.launch(d, STREAM, colors, accum, seg, CAMS[cam], ENVS[0])
            ib = b.launch(d, STREAM, colors, accum, seg, CAMS[cam], ENVS[0])
            assert a.last_ops == b.last_ops, (a.kernel_order(), b.kernel_order())
            assert _rows(a) == _rows(b)
            assert ia == ib
        assert any(op[0] == KERNEL for op in a.last_ops) and {WRITE, ATOMIC, READ} <= {r[2] for r in _rows(a)}
    finally:
        a.close()
        b.close()
