"""The planner's side of a pass over a list of pixels (rtc_render_pixels_async; rtc_plan.h plan_query), on the
CPU through rtc_plan_sim_render_pixels: one kernel (number 17) on the caller's stream that reads the current generation of
the scene records and the caller's list (resource 20), reads the frame's accumulator and RNG states when the pass continues
a frame, writes both, writes the Color and adds to the caller's counter where asked for -- the accumulator, the states and
the Color under the resources a launch's footprint gives them, so that tests/test_plan.py's checker (vector clocks over the
planned operations, unchanged) orders a pixel pass against the whole passes of the same frame -- and a planner state that is
the same afterwards.  No reference counterpart (main.c:263-304 renders whole frames only)."""
from __future__ import annotations

import random

import numpy as np
import pytest

import raytracingc_amd as rt
import test_plan
from raytracingc_amd._abi import RTC_EINVAL
from test_plan import ATOMIC, CAMS, ENVS, KERNEL, KNAMES, OVERLAP, READ, RES_NAMES, WRITE, _desc, _random_launch
from test_plan_trace_paths import PathScenario, _random_paths
from test_plan_trace_rays import STREAM

# rtc_plan.h Kernel and Res after the ones tests/test_plan.py names
KN = KNAMES + ["regroup_centroids", "regroup_level", "regroup_index", "render_pixels"]
RES = RES_NAMES + ["membership", "regroup_scratch", "pixel_list"]
K_PIXELS = KN.index("render_pixels")
R_COLORS, R_ACCUM, R_SEG, R_RNG, R_GEN, R_LIST = (RES.index(n) for n in ("colors", "accum", "caller_segments", "rng_state",
                                                                         "scene_gen", "pixel_list"))
assert (K_PIXELS, R_COLORS, R_ACCUM, R_SEG, R_RNG, R_GEN, R_LIST) == (17, 5, 6, 7, 8, 9, 20)
NO_CULL, WAVE = rt.RTC_F_NO_CLUSTER_CULL, rt.RTC_F_WAVE_PER_RAY
LISTS = (0x210000, 0x218000)  # two lists
COLORS, ACCUM, STATE, SEG = 0x1000, 0xA000, 0xC000, 0x120000  # one frame's buffers


@pytest.fixture(autouse=True)
def _names(monkeypatch):
    """The checker reports a hazard by name: let it name this file's kernel and resource."""
    monkeypatch.setattr(test_plan, "KNAMES", KN)
    monkeypatch.setattr(test_plan, "RES_NAMES", RES)


class PixelScenario(PathScenario):
    """test_plan_trace_paths.PathScenario (launches, passes, updates, first-hit launches, ray and path queries) plus pixel
    passes; `log` keeps what every other step planned, for the comparison with the run without pixel passes."""

    def __init__(self, tri_count):
        super().__init__(tri_count)
        self.pixel_passes = 0

    def pixels(self, stream, pixels, colors, accum, rng, segments=0, first=0, flags=0, order_streams=True):
        caller = ("caller", stream)
        if order_streams and self.last_caller is not None and self.last_caller != caller:  # (one stream at a time)
            self.model.record(self.last_caller, ("caller-switch-x", self.n, self.pixel_passes))
            self.model.wait(caller, ("caller-switch-x", self.n, self.pixel_passes))
        self.last_caller = caller
        rc = self.L.rtc_plan_sim_render_pixels(self.h, stream, pixels, colors, accum, rng, segments, first, flags, self.ops,
                                               64, self.fp, 256)
        assert rc > 0, rc
        nops, nfp = rc & 0xFF, rc >> 8
        fps = np.frombuffer(self.fp, dtype=np.uint64, count=6 * nfp).reshape(nfp, 6).copy()
        assert [int(v) for v in fps[-1]] == [2**64 - 1, 0, int(fps[-1][2]), 0, 0, 0]
        ops = [tuple(int(v) for v in self.ops[4 * i: 4 * i + 4]) for i in range(nops)]
        assert ops == [(KERNEL, 0, -1, K_PIXELS)], "one kernel on the caller's stream: no wait, no record, no event"
        o = self.model.run(caller)
        rows = []
        for row in fps[:-1]:
            i, res, acc, ident, lo, hi = (int(v) for v in row)
            assert i == 0
            self.accesses.append((o, res, acc, ident, lo, hi, ("pixels", self.pixel_passes), self.n, K_PIXELS))
            rows.append((res, acc, ident, lo, hi))
        self.pixel_passes += 1
        return {"gen": int(fps[-1][2]), "rows": rows}

    def launch(self, *a, **kw):
        n0 = len(self.log)
        got = super().launch(*a, **kw)
        # (the parent's log entry, without the pixel passes' rows: they carry the number of the launch after them)
        kind, g, ops, fps, regions = self.log.pop()
        assert len(self.log) == n0
        mine = {tuple(int(v) for v in x[1:6]) for x in self.accesses if x[7] == self.n - 1 and x[8] == K_PIXELS}
        own = tuple(tuple(int(v) for v in x[1:6]) for x in self.accesses
                    if x[7] == self.n - 1 and x[8] not in (11, 12, K_PIXELS))
        assert set(own) | mine >= set(fps)
        self.log.append((kind, g, ops, own, regions))
        return got

    def generation_read(self):
        ids = {a[3] for a in self.accesses
               if a[7] == self.n - 1 and a[1] == R_GEN and KN[a[8]] not in ("refit", "trace_rays", "trace_paths",
                                                                             "render_pixels")}
        assert len(ids) == 1, ids
        return ids.pop()


def _want(gen, lst, colors, accum, rng, segments, first):
    want = [(R_GEN, READ, gen, 0, 1), (R_LIST, READ, lst, 0, 1)]
    want += [(R_ACCUM, READ, accum, 0, 1), (R_RNG, READ, rng, 0, 1)] if first > 0 else []
    want += [(R_ACCUM, WRITE, accum, 0, 1), (R_RNG, WRITE, rng, 0, 1)]
    want += [(R_COLORS, WRITE, colors, 0, 1)] if colors else []
    want += [(R_SEG, ATOMIC, 0, 0, 1)] if segments else []
    return want


@pytest.mark.parametrize("flags", [0, NO_CULL, WAVE, NO_CULL | WAVE])
@pytest.mark.parametrize("segments", [0, SEG])
@pytest.mark.parametrize("colors", [0, COLORS])
@pytest.mark.parametrize("first", [0, 1, 5])
def test_footprint(first, colors, segments, flags):
    """Kernel 17 and exactly these rows in this order: the current generation read, the list read, the accumulator and the
    states read only when the pass continues a frame, both written, the Color written where asked for, the caller's
    counter added to atomically where asked for; no scratch, primary record or counter set.  The flags change the kernel
    behind the number alone."""
    sc = PixelScenario(120)
    try:
        got = sc.pixels(STREAM, LISTS[0], colors, ACCUM, STATE, segments, first, flags)
        assert got["gen"] == 0
        assert got["rows"] == _want(0, LISTS[0], colors, ACCUM, STATE, segments, first)
        # a pipelined frame in flight (on a cull stream and the side stream) into other buffers does not concern it
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x2000, 0, False, CAMS[0], ENVS[0])
        again = sc.pixels(STREAM, LISTS[1], colors, ACCUM, STATE, segments, first, flags)
        assert again["rows"] == _want(0, LISTS[1], colors, ACCUM, STATE, segments, first)
        assert sc.hazards() == []
    finally:
        sc.close()


def test_the_frame_buffers_carry_a_launch_s_resources():
    """The whole pass of the same frame names the accumulator, the states and the Color by the same (resource, id): the
    checker orders the two by the caller's stream, and finds them unordered when the pixel pass strays to another one."""
    sc = PixelScenario(120)
    try:
        d = _desc(64, 40, 12, 0, 1, 0, 0)
        sc.sample_pass(d, STREAM, COLORS, ACCUM, STATE, 0, 5, CAMS[0], ENVS[0])
        whole = {(a[1], a[3]) for a in sc.accesses if a[7] == sc.n - 1}
        assert {(R_COLORS, COLORS), (R_ACCUM, ACCUM), (R_RNG, STATE)} <= whole
        sc.pixels(STREAM, LISTS[0], COLORS, ACCUM, STATE, 0, 5)
        sc.sample_pass(d, STREAM, COLORS, ACCUM, STATE, 5, 7, CAMS[0], ENVS[0])
        assert sc.hazards() == []
        sc.pixels(0x7f002000, LISTS[0], COLORS, ACCUM, STATE, 0, 5, order_streams=False)
        hz = sc.hazards(limit=100)
        assert {h[0] for h in hz} == {"colors", "accum", "rng_state"}, hz
        assert all("render_pixels" in (h[2][1], h[3][1]) for h in hz)
    finally:
        sc.close()


def test_a_pass_reads_the_generation_the_updates_made_current():
    sc = PixelScenario(300)
    try:
        q = lambda: sc.pixels(STREAM, LISTS[0], COLORS, ACCUM, STATE, SEG, 3)  # noqa: E731
        assert q()["gen"] == 0
        assert sc.update(STREAM)["writes"] == 1
        assert q()["gen"] == 1
        assert sc.update(STREAM)["writes"] == 0
        got = q()
        assert got["gen"] == 0 and got["rows"][0] == (R_GEN, READ, 0, 0, 1), "after two updates: generation 0 again"
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x2000, 0, False, CAMS[0], ENVS[0])
        q()
        assert sc.update(STREAM)["writes"] == 1
        assert q()["gen"] == 1
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x3000, 0, False, CAMS[0], ENVS[0])
        assert sc.generation_read() == 1
        assert sc.hazards() == []
        # a stray pass races with the update that rewrites the generation it reads
        sc.pixels(0x7f002000, LISTS[1], 0, 0xA800, 0xC800, 0, 0, order_streams=False)
        sc.last_caller = ("caller", STREAM)
        sc.update(STREAM)
        sc.update(STREAM)
        assert {h[0] for h in sc.hazards(limit=50)} == {"scene_gen"}
    finally:
        sc.close()


def _random_pixels(rng):
    """(list, colors, accum, rng, segments, first, flags) of one of two frames"""
    f = rng.choice([0, 0x800])
    return (rng.choice(LISTS), rng.choice([0, COLORS + f]), ACCUM + f, STATE + f, SEG if rng.random() < 0.4 else 0,
            rng.choice([0, 3, 3]), rng.choice([0, NO_CULL, WAVE]))


def _sequences(seed, pixels, scenes=10, steps=20):
    """Joined and RTC_F_OVERLAP launches, whole frames and row shares, passes of the two frames the pixel passes work on,
    path queries, updates, one or two caller streams -- and, with `pixels`, pixel passes before steps and after updates,
    drawn from a generator of their own so that the rest of the sequence is the same with and without them."""
    rng, prng, xrng = random.Random(31000 + seed), random.Random(33000 + seed), random.Random(37000 + seed)
    shapes = [(1920, 1080), (640, 360), (256, 256), (1000, 700)]
    for _ in range(scenes):
        sc = PixelScenario(rng.choice([12, 120, 300, 5208]))
        if rng.random() < 0.33:
            assert sc.L.rtc_plan_sim_set_spheres(sc.h, rng.choice([1, 5, 40]), rng.randrange(2)) == 0
        streams = [rng.choice([0, 0x7f001000, 0x7f002000])]
        if rng.random() < 0.3:
            streams.append(rng.choice([0, 0x7f003000]))
        try:
            shape = rng.choice(shapes)
            for _ in range(steps):
                st = rng.choice(streams)
                for _ in range(xrng.choice([0, 1, 1, 2]) if pixels else 0):
                    sc.pixels(xrng.choice(streams), *_random_pixels(xrng))
                for _ in range(prng.choice([0, 0, 1])):
                    sc.paths(prng.choice(streams), *_random_paths(prng))
                if rng.random() < 0.2:
                    sc.update(st)
                    if pixels and xrng.random() < 0.5:  # between an update and the launch after it
                        sc.pixels(st, *_random_pixels(xrng))
                if rng.random() < 0.15:
                    shape = rng.choice(shapes)
                d = _random_launch(rng, shape)
                if rng.random() < 0.5:
                    d.trianglesOnly = 0
                if rng.random() < 0.4:  # a whole pass of one of the frames: joined, with its accumulator and states
                    d.flags &= ~OVERLAP
                    f = rng.choice([0, 0x800])
                    first = rng.randrange(d.spp)
                    sc.sample_pass(d, st, COLORS + f, ACCUM + f, STATE + f, first, rng.randint(1, d.spp - first),
                                   rng.choice(CAMS), rng.choice(ENVS))
                    continue
                # (other buffers than the two frames': a pixel pass waits for nothing, so a frame it works on is not the target
                # of a pipelined launch still in flight -- rtc.h)
                colors = rng.choice([0x2000, 0x3000, 0x4000])
                seg = not (d.flags & OVERLAP) and rng.random() < 0.2
                sc.launch(d, st, colors, rng.choice([0, 0, 0, 0x9000 + colors]), seg, rng.choice(CAMS), rng.choice(ENVS))
            yield sc
        finally:
            sc.close()


@pytest.mark.parametrize("seed", range(8))
def test_random_sequences_with_pixel_passes_are_race_free_and_leave_the_plans_alone(seed):
    """No unordered pair of conflicting kernels with the pixel passes in; and every launch, pass, path query and update
    plans exactly what it plans in the same sequence without them: the planner's state after a pixel pass is its state
    before."""
    passes = overlapped = 0
    for with_x, without_x in zip(_sequences(seed, True), _sequences(seed, False)):
        hz = with_x.hazards()
        assert not hz, f"unordered conflicting kernels: {hz}"
        assert without_x.pixel_passes == 0 and without_x.hazards() == []
        assert with_x.n == without_x.n == 20
        assert with_x.log == without_x.log
        passes += with_x.pixel_passes
        overlapped += sum(1 for e in with_x.log if e[0] == "launch" and e[1]["overlap"])
    assert passes > 100 and overlapped > 20


@pytest.mark.parametrize("what", ["no list", "no accumulator", "no states", "negative first", "tile cull flag",
                                  "overlap flag", "debug flag", "null sim", "null ops"])
def test_refusals(what):
    """RTC_EINVAL where the entry point refuses, as far as the planner sees it; a refused pass plans nothing and changes
    nothing."""
    sc = PixelScenario(120)
    try:
        ok = dict(sim=sc.h, pixels=LISTS[0], accum=ACCUM, rng=STATE, first=0, flags=0, ops=sc.ops)
        bad = {"no list": dict(pixels=0), "no accumulator": dict(accum=0), "no states": dict(rng=0),
               "negative first": dict(first=-1), "tile cull flag": dict(flags=rt.RTC_F_NO_TILE_CULL),
               "overlap flag": dict(flags=WAVE | OVERLAP), "debug flag": dict(flags=rt.RTC_F_DEBUG_BOUNCES),
               "null sim": dict(sim=None), "null ops": dict(ops=None)}[what]
        a = dict(ok, **bad)
        assert sc.L.rtc_plan_sim_render_pixels(a["sim"], STREAM, a["pixels"], COLORS, a["accum"], a["rng"], 0, a["first"],
                                               a["flags"], a["ops"], 64, sc.fp, 256) == RTC_EINVAL
        sc.launch(_desc(64, 40, 4, 0, 1, 0, 0), STREAM, 0x2000, 0, False, CAMS[0], ENVS[0])
        assert "chain" in [k for k, _ in sc.kernel_order()]
        assert sc.pixels(STREAM, LISTS[0], COLORS, ACCUM, STATE)["gen"] == 0
    finally:
        sc.close()
