"""The planner's side of a path query (rtc_trace_paths_async; rtc_plan.h plan_query), on the CPU through
rtc_plan_sim_trace_paths: one kernel (number 12) on the caller's stream that reads the current generation of the scene
records, the caller's rays and seeds (and the radiance, when the call continues an accumulation) and writes the radiance,
the seeds and the segment counter asked for, and a planner state that is the same afterwards.  tests/test_plan.py's checker
(vector clocks over the planned operations, unchanged) covers it beside pipelined and joined launches, passes, first-hit
launches, ray queries and updates -- tests/test_plan_trace_rays.py's construction, by import: the random sequences are race
free, and every other operation plans operation for operation, footprint row for footprint row and region for region what it
plans in the same sequence without the path queries.  No reference counterpart (main.c:263-304 renders frames only)."""
from __future__ import annotations

import random

import numpy as np
import pytest

import raytracingc_amd as rt
from raytracingc_amd._abi import RTC_EINVAL
from test_plan import ATOMIC, CAMS, ENVS, KERNEL, KNAMES as KN, OVERLAP, READ, RES_NAMES as RES, WRITE, _desc, _random_launch
from test_plan_first_hit import HitScenario, _random_first_hit
from test_plan_trace_rays import RAYS, STREAM, TraceScenario, _random_query

R_SEG, R_GEN, R_RAYS = RES.index("caller_segments"), RES.index("scene_gen"), RES.index("rays")
R_SEEDS, R_RAD = RES.index("seeds"), RES.index("radiance")
K_RAYS, K_PATHS = KN.index("trace_rays"), KN.index("trace_paths")
assert (R_SEG, R_GEN, R_RAYS, R_SEEDS, R_RAD, K_RAYS, K_PATHS) == (7, 9, 11, 14, 15, 11, 12)
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
SEEDS = (0xF0000, 0xF8000)   # two seed buffers
RADS = (0x110000, 0x118000)  # two radiance buffers
SEG = 0x120000


class PathScenario(TraceScenario):
    """test_plan_trace_rays.TraceScenario (launches, passes, updates, first-hit launches, ray queries) plus path queries,
    with this file's kernel and resource names; `log` keeps what every other step planned -- ray queries included -- for
    the comparison with the run without path queries."""

    def __init__(self, tri_count):
        super().__init__(tri_count)
        self.path_queries = 0

    def paths(self, stream, rays, seeds, radiance, seeds_out=0, segments=0, first=0, flags=0, order_streams=True):
        caller = ("caller", stream)
        if order_streams and self.last_caller is not None and self.last_caller != caller:  # (one stream at a time)
            self.model.record(self.last_caller, ("caller-switch-p", self.n, self.path_queries))
            self.model.wait(caller, ("caller-switch-p", self.n, self.path_queries))
        self.last_caller = caller
        rc = self.L.rtc_plan_sim_trace_paths(self.h, stream, rays, seeds, radiance, seeds_out, segments, first, flags,
                                             self.ops, 64, self.fp, 256)
        assert rc > 0, rc
        nops, nfp = rc & 0xFF, rc >> 8
        fps = np.frombuffer(self.fp, dtype=np.uint64, count=6 * nfp).reshape(nfp, 6).copy()
        assert fps[-1][0] == np.uint64(2**64 - 1)
        ops = [tuple(int(v) for v in self.ops[4 * i: 4 * i + 4]) for i in range(nops)]
        assert ops == [(KERNEL, 0, -1, K_PATHS)], "one kernel on the caller's stream: no wait, no record, no event"
        o = self.model.run(caller)
        rows = []
        for row in fps[:-1]:
            i, res, acc, ident, lo, hi = (int(v) for v in row)
            assert i == 0
            self.accesses.append((o, res, acc, ident, lo, hi, ("paths", self.path_queries), self.n, K_PATHS))
            rows.append((res, acc, ident, lo, hi))
        self.path_queries += 1
        return {"gen": int(fps[-1][2]), "rows": rows}

    def trace(self, *a, **kw):
        got = super().trace(*a, **kw)
        self.log.append(("trace", got))
        return got

    def launch(self, *a, **kw):
        got = HitScenario.launch(self, *a, **kw)  # (TraceScenario.launch's log entry, without either query's rows)
        fps = [tuple(int(v) for v in x[1:6]) for x in self.accesses if x[7] == self.n - 1 and x[8] not in (K_RAYS, K_PATHS)]
        self.log.append(("launch", got, tuple(self.last_ops), tuple(fps), self.regions()))
        return got

    def generation_read(self):
        """The generation the last launch's kernels read (a query before it carries the same launch number: left out)."""
        ids = {a[3] for a in self.accesses
               if a[7] == self.n - 1 and a[1] == R_GEN and KN[a[8]] not in ("refit", "trace_rays", "trace_paths")}
        assert len(ids) == 1, ids
        return ids.pop()


def _random_paths(rng):
    """(rays, seeds, radiance, seeds_out, segments, first, flags): the ray buffers of the sequence's ray queries, one of two
    seed and radiance buffers, the seeds in place, into the other buffer or not at all, with or without the counter, a first
    call or a continuation, with or without RTC_F_NO_CLUSTER_CULL."""
    seeds = rng.choice(SEEDS)
    out = rng.choice([0, seeds, SEEDS[0], SEEDS[1]])
    return (rng.choice(RAYS), seeds, rng.choice(RADS), out, SEG if rng.random() < 0.4 else 0, rng.choice([0, 0, 3]),
            NO_CULL if rng.random() < 0.3 else 0)


def _sequences(seed, paths, scenes=15, steps=24):
    """tests/test_plan_trace_rays.py's sequences with their ray queries in -- joined and RTC_F_OVERLAP launches, whole
    frames and row shares, passes, first-hit launches, ray queries, updates, one or two caller streams -- and, with
    `paths`, path queries before and after steps, drawn from a generator of their own so that the rest of the sequence is
    the same with and without them."""
    rng, qrng, prng = random.Random(13000 + seed), random.Random(17000 + seed), random.Random(19000 + seed)
    shapes = [(1920, 1080), (3840, 2160), (640, 360), (256, 256), (1000, 700)]
    for _ in range(scenes):
        sc = PathScenario(rng.choice([12, 120, 300, 5208]))
        if rng.random() < 0.33:
            assert sc.L.rtc_plan_sim_set_spheres(sc.h, rng.choice([1, 5, 40]), rng.randrange(2)) == 0
        streams = [rng.choice([0, 0x7f001000, 0x7f002000])]
        if rng.random() < 0.3:
            streams.append(rng.choice([0, 0x7f003000]))
        try:
            shape = rng.choice(shapes)
            for _ in range(steps):
                st = rng.choice(streams)
                for _ in range(prng.choice([0, 0, 1, 1, 2]) if paths else 0):
                    sc.paths(prng.choice(streams), *_random_paths(prng))
                for _ in range(qrng.choice([0, 0, 1, 1, 2])):
                    sc.trace(qrng.choice(streams), *_random_query(qrng))
                if rng.random() < 0.2:
                    sc.update(st)
                    if paths and prng.random() < 0.5:  # between an update and the launch after it
                        sc.paths(st, *_random_paths(prng))
                    if qrng.random() < 0.5:
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
def test_random_sequences_with_path_queries_are_race_free_and_leave_the_plans_alone(seed):
    """No unordered pair of conflicting kernels with the path queries in; and every launch, pass, first-hit launch, ray
    query and update plans exactly what it plans in the same sequence without them: the planner's state after a path
    query is its state before."""
    queries = overlapped = rays = 0
    for with_p, without_p in zip(_sequences(seed, True), _sequences(seed, False)):
        hz = with_p.hazards()
        assert not hz, f"unordered conflicting kernels: {hz}"
        assert without_p.path_queries == 0 and without_p.hazards() == []
        assert with_p.n == without_p.n == 24
        assert with_p.log == without_p.log
        queries += with_p.path_queries
        rays += with_p.queries
        overlapped += sum(1 for e in with_p.log if e[0] == "launch" and e[1]["overlap"])
    assert queries > 100 and rays > 100 and overlapped > 30


@pytest.mark.parametrize("flags", [0, NO_CULL])
@pytest.mark.parametrize("segments", [0, SEG])
@pytest.mark.parametrize("seeds_out", [0, SEEDS[0], SEEDS[1]])
@pytest.mark.parametrize("first", [0, 1, 5])
def test_footprint(first, seeds_out, segments, flags):
    """Kernel 12 and exactly these rows in this order: the current generation read, the rays read, the seeds read, the
    radiance read only when the call continues an accumulation, the radiance written, the seeds written into the buffer
    asked for (the seed buffer itself: in place), the caller's counter added to atomically; no scratch, primary record,
    counter set, colour or accumulator."""
    sc = PathScenario(120)
    try:
        got = sc.paths(STREAM, RAYS[0], SEEDS[0], RADS[0], seeds_out, segments, first, flags)
        assert got["gen"] == 0
        want = [(R_GEN, READ, 0, 0, 1), (R_RAYS, READ, RAYS[0], 0, 1), (R_SEEDS, READ, SEEDS[0], 0, 1)]
        want += [(R_RAD, READ, RADS[0], 0, 1)] if first > 0 else []
        want += [(R_RAD, WRITE, RADS[0], 0, 1)]
        want += [(R_SEEDS, WRITE, seeds_out, 0, 1)] if seeds_out else []
        want += [(R_SEG, ATOMIC, 0, 0, 1)] if segments else []
        assert got["rows"] == want
        # a pipelined frame in flight (on a cull stream and the side stream) does not concern it: no wait either way
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        again = sc.paths(STREAM, RAYS[1], SEEDS[1], RADS[1], seeds_out, segments, first, flags)
        assert again["rows"][1:3] == [(R_RAYS, READ, RAYS[1], 0, 1), (R_SEEDS, READ, SEEDS[1], 0, 1)]
        assert len(again["rows"]) == len(want)
        assert sc.hazards() == []
    finally:
        sc.close()


def test_a_query_reads_the_generation_the_updates_made_current():
    sc = PathScenario(300)
    try:
        q = lambda: sc.paths(STREAM, RAYS[0], SEEDS[0], RADS[0], SEEDS[0], SEG)  # noqa: E731
        assert q()["gen"] == 0
        assert sc.update(STREAM)["writes"] == 1
        assert q()["gen"] == 1
        assert sc.update(STREAM)["writes"] == 0
        got = q()
        assert got["gen"] == 0 and got["rows"][0] == (R_GEN, READ, 0, 0, 1), "after two updates: generation 0 again"
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        q()
        assert sc.update(STREAM)["writes"] == 1
        assert q()["gen"] == 1
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x2000, 0, False, CAMS[0], ENVS[0])
        assert sc.generation_read() == 1
        # a joined launch that counts segments and a query that adds to the same counter: ordered by the stream
        sc.launch(_desc(640, 360, 4, 0, 1, 0, 0), STREAM, 0x1000, 0, True, CAMS[0], ENVS[0])
        q()
        assert sc.hazards() == []
    finally:
        sc.close()


def test_the_checker_sees_the_query():
    """Not vacuous: a path query moved to another stream without the order a caller owes (one stream at a time) races
    with the update that rewrites the generation it reads and with the query that writes the same radiance and seeds
    (the rays are only read: they race with nothing)."""
    sc = PathScenario(120)
    try:
        sc.update(STREAM)
        sc.paths(STREAM, RAYS[0], SEEDS[0], RADS[0], SEEDS[0], 0, 0)
        sc.paths(0x7f002000, RAYS[0], SEEDS[0], RADS[0], SEEDS[0], 0, 3, order_streams=False)
        sc.last_caller = ("caller", STREAM)  # (the update stays where the caller's order is)
        sc.update(STREAM)
        sc.update(STREAM)  # writes generation 1, which the stray query reads
        hz = sc.hazards(limit=50)
        assert {h[0] for h in hz} == {"radiance", "seeds", "scene_gen"}, hz
        assert all("trace_paths" in (h[2][1], h[3][1]) for h in hz)
    finally:
        sc.close()


@pytest.mark.parametrize("what", ["no rays", "no seeds", "no radiance", "negative first", "tile cull flag", "overlap flag",
                                  "debug flag", "null sim"])
def test_refusals(what):
    """RTC_EINVAL where the entry point refuses; a refused query plans nothing and changes nothing."""
    sc = PathScenario(120)
    try:
        ok = dict(sim=sc.h, rays=RAYS[0], seeds=SEEDS[0], radiance=RADS[0], first=0, flags=0)
        bad = {"no rays": dict(rays=0), "no seeds": dict(seeds=0), "no radiance": dict(radiance=0),
               "negative first": dict(first=-1), "tile cull flag": dict(flags=rt.RTC_F_NO_TILE_CULL),
               "overlap flag": dict(flags=NO_CULL | OVERLAP), "debug flag": dict(flags=rt.RTC_F_DEBUG_BOUNCES),
               "null sim": dict(sim=None)}[what]
        a = dict(ok, **bad)
        assert sc.L.rtc_plan_sim_trace_paths(a["sim"], STREAM, a["rays"], a["seeds"], a["radiance"], 0, 0, a["first"],
                                             a["flags"], sc.ops, 64, sc.fp, 256) == RTC_EINVAL
        sc.launch(_desc(64, 40, 4, 0, 1, 0, 0), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        assert "chain" in [k for k, _ in sc.kernel_order()]
        assert sc.paths(STREAM, RAYS[0], SEEDS[0], RADS[0])["gen"] == 0
    finally:
        sc.close()
