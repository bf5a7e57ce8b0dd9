"""The planner's side of a ray query (rtc_trace_rays_async; rtc_plan.h plan_query), on the CPU through
rtc_plan_sim_trace_rays: one kernel (number 11) on the caller's stream that reads the current generation of the scene
records and the caller's rays and writes the caller's hit buffers, and a planner state that is the same afterwards.
tests/test_plan.py's checker (vector clocks over the planned operations, unchanged) covers it beside pipelined and joined
launches, passes, first-hit launches and updates: the random sequences are race free, every other launch and update plans
operation for operation, footprint row for footprint row and region for region as it does in the same sequence without the
queries, the footprint is exactly the rows stated, and a query after updates names the generation they made current.  No
reference counterpart (main.c:263-304 renders frames only)."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import raytracingc_amd as rt
from raytracingc_amd._abi import RTC_EINVAL
from test_plan import CAMS, ENVS, KERNEL, KNAMES as KN, OVERLAP, READ, RES_NAMES as RES, WRITE, _desc, _random_launch
from test_plan_first_hit import IDS, HitScenario, _random_first_hit

R_GEN, R_HIT, R_RAYS = RES.index("scene_gen"), RES.index("hit"), RES.index("rays")
K_TRACE = KN.index("trace_rays")
assert (R_GEN, R_HIT, R_RAYS, K_TRACE) == (9, 10, 11, 11)
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
STREAM = 0x7f001000
RAYS = (0xE0000, 0xE8000)  # two ray buffers


class TraceScenario(HitScenario):
    """test_plan_first_hit.HitScenario (launches, passes, updates, first-hit launches) plus ray queries, with this file's
    kernel and resource names; `log` keeps what every step planned, for the comparison with the run without queries."""

    def __init__(self, tri_count):
        super().__init__(tri_count)
        self.queries = 0
        self.log = []

    def trace(self, stream, rays, ids, flags=0, order_streams=True):
        caller = ("caller", stream)
        if order_streams and self.last_caller is not None and self.last_caller != caller:  # (one stream at a time)
            self.model.record(self.last_caller, ("caller-switch-q", self.n, self.queries))
            self.model.wait(caller, ("caller-switch-q", self.n, self.queries))
        self.last_caller = caller
        rc = self.L.rtc_plan_sim_trace_rays(self.h, stream, rays, (C.c_ulonglong * 4)(*ids), flags, self.ops, 64, self.fp, 256)
        assert rc > 0, rc
        nops, nfp = rc & 0xFF, rc >> 8
        fps = np.frombuffer(self.fp, dtype=np.uint64, count=6 * nfp).reshape(nfp, 6).copy()
        assert fps[-1][0] == np.uint64(2**64 - 1)
        ops = [tuple(int(v) for v in self.ops[4 * i: 4 * i + 4]) for i in range(nops)]
        assert ops == [(KERNEL, 0, -1, K_TRACE)], "one kernel on the caller's stream: no wait, no record, no event"
        o = self.model.run(caller)
        rows = []
        for row in fps[:-1]:
            i, res, acc, ident, lo, hi = (int(v) for v in row)
            assert i == 0
            self.accesses.append((o, res, acc, ident, lo, hi, ("query", self.queries), self.n, K_TRACE))
            rows.append((res, acc, ident, lo, hi))
        self.queries += 1
        return {"gen": int(fps[-1][2]), "rows": rows}

    def launch(self, *a, **kw):
        got = super().launch(*a, **kw)
        fps = [tuple(int(v) for v in x[1:6]) for x in self.accesses if x[7] == self.n - 1 and x[8] != K_TRACE]
        self.log.append(("launch", got, tuple(self.last_ops), tuple(fps), self.regions()))
        return got

    def update(self, stream):
        got = super().update(stream)
        self.log.append(("update", got, tuple(self.last_update_ops)))
        return got

    def generation_read(self):
        """The generation the last launch's kernels read (a query before it carries the same launch number: left out)."""
        ids = {a[3] for a in self.accesses if a[7] == self.n - 1 and a[1] == R_GEN and KN[a[8]] not in ("refit", "trace_rays")}
        assert len(ids) == 1, ids
        return ids.pop()


def _random_query(rng):
    """(rays, ids, flags): one of two ray buffers, a random non-empty subset of the first-hit tests' buffer identities (the
    same ones the first-hit launches of the sequence write), with or without RTC_F_NO_CLUSTER_CULL."""
    base = rng.choice([0, 0x100000])
    ids = [(i + base) if rng.random() < 0.6 else 0 for i in IDS]
    if not any(ids):
        ids[rng.randrange(4)] = IDS[0] + base
    return rng.choice(RAYS), ids, NO_CULL if rng.random() < 0.3 else 0


def _sequences(seed, queries, scenes=15, steps=24):
    """`scenes` scenes x `steps` steps as tests/test_plan_first_hit.py draws them -- joined and RTC_F_OVERLAP launches, whole
    frames and row shares, passes, first-hit launches, updates, one or two caller streams -- and, with `queries`, ray
    queries before and after steps, drawn from a generator of their own so that the rest of the sequence is the same
    with and without them."""
    rng, qrng = random.Random(13000 + seed), random.Random(17000 + seed)
    shapes = [(1920, 1080), (3840, 2160), (640, 360), (256, 256), (1000, 700)]
    for _ in range(scenes):
        sc = TraceScenario(rng.choice([12, 120, 300, 5208]))
        if rng.random() < 0.33:
            assert sc.L.rtc_plan_sim_set_spheres(sc.h, rng.choice([1, 5, 40]), rng.randrange(2)) == 0
        streams = [rng.choice([0, 0x7f001000, 0x7f002000])]
        if rng.random() < 0.3:
            streams.append(rng.choice([0, 0x7f003000]))
        try:
            shape = rng.choice(shapes)
            for _ in range(steps):
                st = rng.choice(streams)
                for _ in range(qrng.choice([0, 0, 1, 1, 2]) if queries else 0):
                    sc.trace(qrng.choice(streams), *_random_query(qrng))
                if rng.random() < 0.2:
                    sc.update(st)
                    if queries and qrng.random() < 0.5:  # between an update and the launch after it
                        sc.trace(st, *_random_query(qrng))
                if rng.random() < 0.15:
                    shape = rng.choice(shapes)
                u = rng.random()
                if u < 0.2:
                    d, ids = _random_first_hit(rng, shape)
                    sc.first_hit(d, st, ids, rng.choice(CAMS))
                    continue
                d = _random_launch(rng, shape)
                if rng.random() < 0.5:
                    d.trianglesOnly = 0
                colors = rng.choice([0x1000, 0x2000, 0x3000])
                if u < 0.35:  # a pass of a progressive frame: joined, with its accumulator and states
                    d.flags &= ~OVERLAP
                    first = rng.randrange(d.spp)
                    sc.sample_pass(d, st, colors, 0x9000 + colors, 0xB000 + colors, first, rng.randint(1, d.spp - first),
                                   rng.choice(CAMS), rng.choice(ENVS))
                    continue
                seg = not (d.flags & OVERLAP) and rng.random() < 0.2
                sc.launch(d, st, colors, rng.choice([0, 0, 0, 0x9000 + colors]), seg, rng.choice(CAMS), rng.choice(ENVS))
            yield sc
        finally:
            sc.close()


@pytest.mark.parametrize("seed", range(20))
def test_random_sequences_with_queries_are_race_free_and_leave_the_plans_alone(seed):
    """No unordered pair of conflicting kernels with the queries in; and every launch, pass, first-hit launch and update
    plans exactly what it plans in the same sequence without them -- slot, streams, operations (waits and records
    included), every footprint row and every bound region: the planner's state after a query is its state before."""
    queries = overlapped = 0
    for with_q, without_q in zip(_sequences(seed, True), _sequences(seed, False)):
        hz = with_q.hazards()
        assert not hz, f"unordered conflicting kernels: {hz}"
        assert without_q.queries == 0 and without_q.hazards() == []
        assert with_q.n == without_q.n == 24
        assert with_q.log == without_q.log
        queries += with_q.queries
        overlapped += sum(1 for e in with_q.log if e[0] == "launch" and e[1]["overlap"])
    assert queries > 100 and overlapped > 30


@pytest.mark.parametrize("flags", [0, NO_CULL])
@pytest.mark.parametrize("ids", [IDS, (IDS[0], 0, 0, 0), (0, IDS[1], 0, IDS[3]), (0, 0, IDS[2], 0)])
def test_footprint(ids, flags):
    """Kernel 11 and exactly these rows: the current generation read, the ray buffer read, one write per buffer asked for
    with that buffer's identity, in that order; no scratch, primary record, counter set, colour or accumulator."""
    sc = TraceScenario(120)
    try:
        got = sc.trace(STREAM, RAYS[0], ids, flags)
        assert got["gen"] == 0
        assert got["rows"] == [(R_GEN, READ, 0, 0, 1), (R_RAYS, READ, RAYS[0], 0, 1)] + \
            [(R_HIT, WRITE, i, 0, 1) for i in ids if i]
        # a pipelined frame in flight (on a cull stream and the side stream) does not concern it: no wait either way
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        again = sc.trace(STREAM, RAYS[1], ids, flags)
        assert again["rows"][1] == (R_RAYS, READ, RAYS[1], 0, 1) and again["rows"][2:] == got["rows"][2:]
        assert sc.hazards() == []
    finally:
        sc.close()


def test_a_query_reads_the_generation_the_updates_made_current():
    sc = TraceScenario(300)
    try:
        assert sc.trace(STREAM, RAYS[0], IDS)["gen"] == 0
        assert sc.update(STREAM)["writes"] == 1
        assert sc.trace(STREAM, RAYS[0], IDS)["gen"] == 1
        assert sc.update(STREAM)["writes"] == 0
        got = sc.trace(STREAM, RAYS[0], IDS)
        assert got["gen"] == 0 and got["rows"][0] == (R_GEN, READ, 0, 0, 1), "after two updates: generation 0 again"
        # queries on both sides of an update of a scene with pipelined frames in flight: the update's waits are its own
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        sc.trace(STREAM, RAYS[0], IDS)
        assert sc.update(STREAM)["writes"] == 1
        assert sc.trace(STREAM, RAYS[1], IDS)["gen"] == 1
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x2000, 0, False, CAMS[0], ENVS[0])
        assert sc.generation_read() == 1
        assert sc.hazards() == []
    finally:
        sc.close()


def test_the_checker_sees_the_query():
    """Not vacuous: a query moved to another stream without the order a caller owes (one stream at a time) races with the
    update that rewrites the generation it reads and with the query that writes the same buffers."""
    sc = TraceScenario(120)
    try:
        sc.update(STREAM)
        sc.trace(STREAM, RAYS[0], IDS)
        sc.trace(0x7f002000, RAYS[0], IDS, order_streams=False)
        sc.last_caller = ("caller", STREAM)  # (the update stays where the caller's order is)
        sc.update(STREAM)
        sc.update(STREAM)  # writes generation 1, which the stray query reads
        hz = sc.hazards(limit=50)
        assert {h[0] for h in hz} == {"hit", "scene_gen"}, hz
        assert all("trace_rays" in (h[2][1], h[3][1]) for h in hz)
    finally:
        sc.close()


@pytest.mark.parametrize("what", ["no rays", "no buffer", "tile cull flag", "overlap flag", "null sim", "null ids"])
def test_refusals(what):
    """RTC_EINVAL where the entry point refuses; a refused query plans nothing and changes nothing."""
    sc = TraceScenario(120)
    try:
        L, ids = sc.L, (C.c_ulonglong * 4)(*IDS)
        args = {"no rays": (sc.h, STREAM, 0, ids, 0), "no buffer": (sc.h, STREAM, RAYS[0], (C.c_ulonglong * 4)(), 0),
                "tile cull flag": (sc.h, STREAM, RAYS[0], ids, rt.RTC_F_NO_TILE_CULL),
                "overlap flag": (sc.h, STREAM, RAYS[0], ids, NO_CULL | OVERLAP), "null sim": (None, STREAM, RAYS[0], ids, 0),
                "null ids": (sc.h, STREAM, RAYS[0], None, 0)}[what]
        assert L.rtc_plan_sim_trace_rays(*args, sc.ops, 64, sc.fp, 256) == RTC_EINVAL
        sc.launch(_desc(64, 40, 4, 0, 1, 0, 0), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        assert "chain" in [k for k, _ in sc.kernel_order()] and "trace_rays" not in [k for k, _ in sc.kernel_order()]
        assert sc.trace(STREAM, RAYS[0], IDS)["gen"] == 0
    finally:
        sc.close()
