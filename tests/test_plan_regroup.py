"""The launch planner with regroups (rtc_plan.h plan_regroup; rtc_scene_regroup_async), driven on the CPU
through rtc_plan_sim_regroup with tests/test_plan.py's checker (vector clocks over the planned operations, no GPU).  A
regroup is an update whose refit is preceded, on the caller's stream, by the kernels that decide the cluster membership:
the centroids (kernel 14), one kernel per level (15) and the index kernel (16), with two resources of their own -- the
membership (18), which only refits read, and the caller's regroup scratch (19).  Checked: random sequences of overlapped
launches, updates, regroups and the three queries are race-free; a regroup between steady pipelined frames waits for
exactly what an update would, never for the frame just enqueued; an update after a regroup reads the membership after
the regroup wrote it; an update's own plan is what it was.  No reference counterpart (main.c:229-243 builds its arrays
once)."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import test_plan
from raytracingc_amd._abi import RTC_EINVAL
from test_plan import CAMS, ENVS, KERNEL, KNAMES, OVERLAP, READ, RES_NAMES, WAIT, WRITE, StreamModel, _desc, _random_launch
from test_plan_occluded import OccScenario, _random_occluded
from test_plan_trace_paths import _random_paths
from test_plan_trace_rays import _random_query
from test_plan_update import EV_GEO_DONE0, EV_SKY_DONE0, UpdateScenario

# rtc_plan.h Kernel and Res after the ones tests/test_plan.py names
KN = KNAMES + ["regroup_centroids", "regroup_level", "regroup_index"]
RES = RES_NAMES + ["membership", "regroup_scratch"]
K_REFIT, K_CENT, K_LEVEL, K_INDEX = KN.index("refit"), KN.index("regroup_centroids"), KN.index("regroup_level"), KN.index("regroup_index")
R_GEN, R_MEMBERS, R_SCRATCH = RES.index("scene_gen"), RES.index("membership"), RES.index("regroup_scratch")
assert (K_REFIT, K_CENT, K_LEVEL, K_INDEX, R_GEN, R_MEMBERS, R_SCRATCH) == (9, 14, 15, 16, 9, 18, 19)
SCRATCH = (0x200000, 0x280000)  # two scratch buffers
STREAM = 0x7f001000


@pytest.fixture(autouse=True)
def _names(monkeypatch):
    """The checker reports a hazard by name: let it name this file's kernels and resources."""
    monkeypatch.setattr(test_plan, "KNAMES", KN)
    monkeypatch.setattr(test_plan, "RES_NAMES", RES)


def levels_of(n):
    """The levels of the median split of n triangles: splits at multiples of 8, the left half the larger."""
    levels, hi = 0, n
    while hi > 8:
        hi = ((hi + 7) // 8 + 1) // 2 * 8
        levels += 1
    return levels


class RegroupScenario(OccScenario):
    """test_plan_occluded.OccScenario (launches, passes, updates, first-hit launches, the three queries) plus
    rtc_plan_sim_regroup."""

    def __init__(self, tri_count):
        super().__init__(tri_count)
        self.tri_count = tri_count
        self.regroups = 0

    def regroup(self, stream, scratch):
        caller = ("caller", stream)
        if self.last_caller is not None and self.last_caller != caller:  # (one stream at a time)
            self.model.record(self.last_caller, ("caller-switch-g", self.n, self.regroups))
            self.model.wait(caller, ("caller-switch-g", self.n, self.regroups))
        self.last_caller = caller
        rc = self.L.rtc_plan_sim_regroup(self.h, stream, scratch, self.ops, 64, self.fp, 256)
        assert rc > 0, rc
        nops, nfp = rc & 0xFF, rc >> 8
        fps = np.frombuffer(self.fp, dtype=np.uint64, count=6 * nfp).reshape(nfp, 6).copy()
        assert fps[-1][0] == np.uint64(2**64 - 1)
        ops = [tuple(int(v) for v in self.ops[4 * i: 4 * i + 4]) for i in range(nops)]
        assert all(st == 0 for _, st, _, _ in ops), "a regroup runs on the caller's stream alone"
        waits = [ev for kind, _, ev, _ in ops if kind == WAIT]
        kernels = [k for kind, _, ev, k in ops if kind == KERNEL]
        levels = int(fps[-1][3])
        assert levels == levels_of(self.tri_count)
        assert ops[:len(waits)] == [(WAIT, 0, ev, -1) for ev in waits], "the waits come first"
        assert ops[len(waits):] == [(KERNEL, 0, -1, k) for k in kernels], "then kernels alone, none with an event"
        assert kernels == [K_CENT] + [K_LEVEL] * levels + [K_INDEX, K_REFIT]
        for ev in waits:
            self.model.wait(caller, ("scene", ev))
        clock = {}
        for i, (kind, _, _, k) in enumerate(ops):
            if kind == KERNEL:
                clock[i] = (self.model.run(caller), k)
        rows = {}
        for row in fps[:-1]:
            i, res, acc, ident, lo, hi = (int(v) for v in row)
            o, k = clock[i]
            self.accesses.append((o, res, acc, ident, lo, hi, ("regroup", self.regroups), self.n, k))
            rows.setdefault(i, []).append((res, acc, ident, lo, hi))
        writes = int(fps[-1][2])
        by_kernel = [rows[i] for i in sorted(rows)]
        s_r, s_w = (R_SCRATCH, READ, scratch, 0, 1), (R_SCRATCH, WRITE, scratch, 0, 1)
        assert by_kernel[0] == [s_w]
        assert by_kernel[1:1 + levels] == [[s_r, s_w]] * levels
        assert by_kernel[-2] == [s_r, (R_MEMBERS, WRITE, 0, 0, 1)]
        assert by_kernel[-1] == [(R_GEN, WRITE, writes, 0, 1), (R_GEN, READ, 1 - writes, 0, 1), (R_MEMBERS, READ, 0, 0, 1)]
        self.regroups += 1
        self.updates += 1
        self.stale = set(range(8))
        self.log.append(("regroup", writes, tuple(ops)))
        return {"writes": writes, "waits": waits, "levels": levels}

    def generation_read(self):
        ids = {a[3] for a in self.accesses if a[7] == self.n - 1 and a[1] == R_GEN and
               KN[a[8]] not in ("refit", "trace_rays", "trace_paths", "occluded")}
        assert len(ids) == 1, ids
        return ids.pop()


def _sequences(seed, scenes=15, steps=24):
    """Random scenes and steps as tests/test_plan_occluded.py draws them -- joined and RTC_F_OVERLAP launches, whole frames
    and row shares, the three queries, one or two caller streams -- with an update or a regroup before a step with
    probability 0.35, sometimes two in a row, and queries between them and the launch after."""
    rng = random.Random(29000 + seed)
    shapes = [(1920, 1080), (3840, 2160), (640, 360), (256, 256), (1000, 700)]
    for _ in range(scenes):
        sc = RegroupScenario(rng.choice([12, 120, 300, 5208]))
        if rng.random() < 0.33:
            assert sc.L.rtc_plan_sim_set_spheres(sc.h, rng.choice([1, 5, 40]), rng.randrange(2)) == 0
        streams = [rng.choice([0, 0x7f001000, 0x7f002000])]
        if rng.random() < 0.3:
            streams.append(rng.choice([0, 0x7f003000]))
        missing = 0
        try:
            shape = rng.choice(shapes)
            for _ in range(steps):
                st = rng.choice(streams)
                for _ in range(rng.choice([0, 0, 1])):
                    sc.occluded(rng.choice(streams), *_random_occluded(rng))
                for _ in range(rng.choice([0, 0, 1])):
                    sc.paths(rng.choice(streams), *_random_paths(rng))
                for _ in range(rng.choice([0, 0, 1])):
                    sc.trace(rng.choice(streams), *_random_query(rng))
                for _ in range(rng.choice([0, 0, 0, 0, 0, 0, 1, 1, 1, 2])):
                    if rng.random() < 0.6:
                        sc.regroup(st, rng.choice(SCRATCH))
                    else:
                        sc.update(st)
                    if rng.random() < 0.5:
                        sc.trace(st, *_random_query(rng))
                if rng.random() < 0.15:
                    shape = rng.choice(shapes)
                d = _random_launch(rng, shape)
                if rng.random() < 0.5:
                    d.trianglesOnly = 0
                seg = not (d.flags & OVERLAP) and rng.random() < 0.2
                colors = rng.choice([0x1000, 0x2000, 0x3000])
                sc.launch(d, st, colors, rng.choice([0, 0, 0, 0x9000 + colors]), seg, rng.choice(CAMS), rng.choice(ENVS))
                missing += sc.prep_missing
            yield sc, missing
        finally:
            sc.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_sequences_with_regroups_are_race_free(seed):
    launches = regroups = 0
    for sc, missing in _sequences(seed):
        launches += sc.n
        regroups += sc.regroups
        hz = sc.hazards()
        assert not hz, f"unordered conflicting kernels: {hz}"
        assert missing == 0, "a launch after a regroup kept primary records of the old triangles"
    assert launches == 15 * 24 and regroups > 40


def test_steady_pipelined_regroups_keep_the_overlap():
    """test_plan_update's steady sequence with a regroup in the update's place: overlapped whole 1080p frames, a regroup
    before each.  Regroup k waits for the slot of frame k - 2, the last reader of the generation it rewrites, and for
    nothing else -- never for frame k - 1, whose kernels are still running."""
    sc = RegroupScenario(3868)
    try:
        d = _desc(1920, 1080, 64, 0, 1, 0, OVERLAP)
        slots = []
        for k in range(20):
            g = sc.regroup(STREAM, SCRATCH[k % 2]) if k % 3 else sc.update(STREAM)
            want = [EV_SKY_DONE0 + slots[k - 2]] if k >= 2 else []
            assert g["waits"] == want, (k, g, slots)
            if k >= 1:
                assert not {EV_SKY_DONE0 + slots[-1], EV_GEO_DONE0 + slots[-1]} & set(g["waits"])
            got = sc.launch(d, STREAM, 0x1000 + 0x1000 * (k % 3), 0, False, CAMS[0], ENVS[0])
            assert got["overlap"] and got["alt"]
            assert sc.generation_read() == g["writes"]
            slots.append(got["slot"])
        assert sc.regroup(STREAM, SCRATCH[0])["waits"] == [EV_SKY_DONE0 + slots[-2]]
        assert sc.regroup(STREAM, SCRATCH[0])["waits"] == [EV_SKY_DONE0 + slots[-1]]
        assert sc.regroup(STREAM, SCRATCH[0])["waits"] == []
        assert sc.hazards() == []
    finally:
        sc.close()


def test_update_after_regroup_reads_the_new_membership():
    """The refit of a later update is ordered after the regroup's write of the membership (one stream, stream order), and
    the checker would see it if it were not: the same accesses replayed with the update on an unordered stream race."""
    sc = RegroupScenario(300)
    try:
        sc.launch(_desc(640, 360, 16, 0, 1, 0, OVERLAP), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        sc.regroup(STREAM, SCRATCH[0])
        writer = [a for a in sc.accesses if a[1] == R_MEMBERS and a[2] == WRITE]
        assert len(writer) == 1 and writer[0][8] == K_INDEX
        # an update's own footprint names no membership (its plan is pinned by the existing tests): the refit's read is the
        # regroup's row, so give the update's refit that row as the executor's kernel has it
        sc.update(STREAM)
        refit = [a for a in sc.accesses if a[8] == K_REFIT][-1]
        sc.accesses.append((refit[0], R_MEMBERS, READ, 0, 0, 1, refit[6], refit[7], K_REFIT))
        assert StreamModel.before(writer[0][0], refit[0])
        assert sc.hazards() == []
        # the same read from a stream nothing orders: a hazard on the membership
        stray = sc.model.run(("caller", 0x7f009000))
        sc.accesses.append((stray, R_MEMBERS, READ, 0, 0, 1, ("stray", 0), sc.n, K_REFIT))
        hz = sc.hazards()
        assert hz and hz[0][0] == "membership"
    finally:
        sc.close()


def test_update_plans_are_unchanged():
    """plan_update's output with regroups in the sequence: every update still plans its waits and one refit with the two
    generation rows -- no membership row, no new kernel."""
    sc = RegroupScenario(120)
    try:
        d = _desc(1000, 700, 4, 0, 1, 0, OVERLAP)
        for k in range(6):
            (sc.regroup(STREAM, SCRATCH[0]) if k % 2 else sc.update(STREAM))
            sc.launch(d, STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        plain = UpdateScenario(120)
        try:
            for k in range(6):
                plain.update(STREAM)
                plain.launch(d, STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
            rows = lambda s: [a[1:6] for a in s.accesses if a[8] == K_REFIT and a[1] != R_MEMBERS]  # noqa: E731
            assert rows(sc) == rows(plain)
        finally:
            plain.close()
    finally:
        sc.close()


def test_refusals():
    sc = RegroupScenario(120)
    try:
        L = sc.L
        assert L.rtc_plan_sim_regroup(None, STREAM, SCRATCH[0], sc.ops, 64, sc.fp, 256) == RTC_EINVAL
        assert L.rtc_plan_sim_regroup(sc.h, STREAM, 0, sc.ops, 64, sc.fp, 256) == RTC_EINVAL
        assert L.rtc_plan_sim_regroup(sc.h, STREAM, SCRATCH[0] + 8, sc.ops, 64, sc.fp, 256) == RTC_EINVAL
        assert L.rtc_plan_sim_regroup(sc.h, STREAM, SCRATCH[0], None, 64, sc.fp, 256) == RTC_EINVAL
        assert sc.update(STREAM)["writes"] == 1, "the refused regroups planned nothing"
    finally:
        sc.close()
    empty = RegroupScenario(0)
    try:
        assert empty.L.rtc_plan_sim_regroup(empty.h, STREAM, SCRATCH[0], empty.ops, 64, empty.fp, 256) == RTC_EINVAL
    finally:
        empty.close()


@pytest.mark.parametrize("n", [1, 8, 9, 16, 17, 120, 3868, 5208])
def test_levels(n):
    sc = RegroupScenario(n)
    try:
        assert sc.regroup(STREAM, SCRATCH[1])["levels"] == levels_of(n)
    finally:
        sc.close()
