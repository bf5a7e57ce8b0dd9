"""The planner's side of an occlusion query (rtc_occluded_async; rtc_plan.h plan_query), on the CPU through
rtc_plan_sim_occluded: one kernel (number 13) on the caller's stream that reads the current generation of the scene
records, the caller's rays and limits and writes the bytes and the counter asked for, and a planner state that is the same
afterwards.  tests/test_plan.py's checker (vector clocks over the planned operations, unchanged) covers it beside pipelined
and joined launches, passes, first-hit launches, ray and path queries and updates -- tests/test_plan_trace_paths.py's
construction, by import: the random sequences are race free, and every other operation plans operation for operation,
footprint row for footprint row and region for region what it plans in the same sequence without the occlusion queries.
No reference counterpart (main.c:263-304 renders frames only)."""
from __future__ import annotations

import random

import numpy as np
import pytest

import raytracingc_amd as rt
from raytracingc_amd._abi import RTC_EINVAL
from test_plan import ATOMIC, CAMS, ENVS, KERNEL, KNAMES as KN, OVERLAP, READ, RES_NAMES as RES, WRITE, _desc, _random_launch
from test_plan_first_hit import HitScenario, _random_first_hit
from test_plan_trace_paths import PathScenario, _random_paths
from test_plan_trace_rays import RAYS, STREAM, _random_query

R_SEG, R_GEN, R_RAYS = RES.index("caller_segments"), RES.index("scene_gen"), RES.index("rays")
R_TMAX, R_OCC = RES.index("tmax"), RES.index("occluded")
K_RAYS, K_PATHS, K_OCC = KN.index("trace_rays"), KN.index("trace_paths"), KN.index("occluded")
assert (R_SEG, R_GEN, R_RAYS, R_TMAX, R_OCC, K_RAYS, K_PATHS, K_OCC) == (7, 9, 11, 16, 17, 11, 12, 13)
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
TMAXS = (0x130000, 0x138000)  # two limit buffers
OCCS = (0x140001, 0x148003)   # two byte buffers (any alignment)
COUNT = 0x150000


class OccScenario(PathScenario):
    """test_plan_trace_paths.PathScenario (launches, passes, updates, first-hit launches, ray and path queries) plus
    occlusion queries, with this file's kernel and resource names; `log` keeps what every other step planned -- both other
    queries included -- for the comparison with the run without occlusion queries."""

    def __init__(self, tri_count):
        super().__init__(tri_count)
        self.occ_queries = 0

    def occluded(self, stream, rays, tmax=0, occluded=0, count=0, flags=0, order_streams=True):
        caller = ("caller", stream)
        if order_streams and self.last_caller is not None and self.last_caller != caller:  # (one stream at a time)
            self.model.record(self.last_caller, ("caller-switch-o", self.n, self.occ_queries))
            self.model.wait(caller, ("caller-switch-o", self.n, self.occ_queries))
        self.last_caller = caller
        rc = self.L.rtc_plan_sim_occluded(self.h, stream, rays, tmax, occluded, count, flags, self.ops, 64, self.fp, 256)
        assert rc > 0, rc
        nops, nfp = rc & 0xFF, rc >> 8
        fps = np.frombuffer(self.fp, dtype=np.uint64, count=6 * nfp).reshape(nfp, 6).copy()
        assert fps[-1][0] == np.uint64(2**64 - 1)
        ops = [tuple(int(v) for v in self.ops[4 * i: 4 * i + 4]) for i in range(nops)]
        assert ops == [(KERNEL, 0, -1, K_OCC)], "one kernel on the caller's stream: no wait, no record, no event"
        o = self.model.run(caller)
        rows = []
        for row in fps[:-1]:
            i, res, acc, ident, lo, hi = (int(v) for v in row)
            assert i == 0
            self.accesses.append((o, res, acc, ident, lo, hi, ("occluded", self.occ_queries), self.n, K_OCC))
            rows.append((res, acc, ident, lo, hi))
        self.occ_queries += 1
        return {"gen": int(fps[-1][2]), "rows": rows}

    def paths(self, *a, **kw):
        got = super().paths(*a, **kw)
        self.log.append(("paths", got))
        return got

    def launch(self, *a, **kw):
        got = HitScenario.launch(self, *a, **kw)  # (the log entry without any query's rows)
        fps = [tuple(int(v) for v in x[1:6]) for x in self.accesses
               if x[7] == self.n - 1 and x[8] not in (K_RAYS, K_PATHS, K_OCC)]
        self.log.append(("launch", got, tuple(self.last_ops), tuple(fps), self.regions()))
        return got

    def generation_read(self):
        """The generation the last launch's kernels read (a query before it carries the same launch number: left out)."""
        ids = {a[3] for a in self.accesses if a[7] == self.n - 1 and a[1] == R_GEN and
               KN[a[8]] not in ("refit", "trace_rays", "trace_paths", "occluded")}
        assert len(ids) == 1, ids
        return ids.pop()


def _random_occluded(rng):
    """(rays, tmax, occluded, count, flags): the ray buffers of the sequence's other queries, limits or none, the bytes,
    the counter or both, with or without RTC_F_NO_CLUSTER_CULL."""
    out = rng.choice([(1, 0), (0, 1), (1, 1)])
    return (rng.choice(RAYS), rng.choice((0,) + TMAXS), rng.choice(OCCS) if out[0] else 0, COUNT if out[1] else 0,
            rng.choice([0, 0, NO_CULL]))


def _sequences(seed, occluded, scenes=15, steps=24):
    """tests/test_plan_trace_paths.py's sequences with their ray and path queries in -- joined and RTC_F_OVERLAP launches,
    whole frames and row shares, passes, first-hit launches, ray and path queries, updates, one or two caller streams --
    and, with `occluded`, occlusion queries before and after steps, drawn from a generator of their own so that the rest
    of the sequence is the same with and without them."""
    rng, qrng, prng = random.Random(13000 + seed), random.Random(17000 + seed), random.Random(19000 + seed)
    orng = random.Random(23000 + seed)
    shapes = [(1920, 1080), (3840, 2160), (640, 360), (256, 256), (1000, 700)]
    for _ in range(scenes):
        sc = OccScenario(rng.choice([12, 120, 300, 5208]))
        if rng.random() < 0.33:
            assert sc.L.rtc_plan_sim_set_spheres(sc.h, rng.choice([1, 5, 40]), rng.randrange(2)) == 0
        streams = [rng.choice([0, 0x7f001000, 0x7f002000])]
        if rng.random() < 0.3:
            streams.append(rng.choice([0, 0x7f003000]))
        try:
            shape = rng.choice(shapes)
            for _ in range(steps):
                st = rng.choice(streams)
                for _ in range(orng.choice([0, 0, 1, 1, 2]) if occluded else 0):
                    sc.occluded(orng.choice(streams), *_random_occluded(orng))
                for _ in range(prng.choice([0, 0, 1])):
                    sc.paths(prng.choice(streams), *_random_paths(prng))
                for _ in range(qrng.choice([0, 0, 1, 1, 2])):
                    sc.trace(qrng.choice(streams), *_random_query(qrng))
                if rng.random() < 0.2:
                    sc.update(st)
                    if occluded and orng.random() < 0.5:  # between an update and the launch after it
                        sc.occluded(st, *_random_occluded(orng))
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
def test_random_sequences_with_occlusion_queries_are_race_free_and_leave_the_plans_alone(seed):
    """No unordered pair of conflicting kernels with the occlusion queries in; and every launch, pass, first-hit launch,
    ray query, path query and update plans exactly what it plans in the same sequence without them: the planner's state
    after an occlusion query is its state before."""
    queries = overlapped = rays = paths = 0
    for with_o, without_o in zip(_sequences(seed, True), _sequences(seed, False)):
        hz = with_o.hazards()
        assert not hz, f"unordered conflicting kernels: {hz}"
        assert without_o.occ_queries == 0 and without_o.hazards() == []
        assert with_o.n == without_o.n == 24
        assert with_o.log == without_o.log
        queries += with_o.occ_queries
        rays += with_o.queries
        paths += with_o.path_queries
        overlapped += sum(1 for e in with_o.log if e[0] == "launch" and e[1]["overlap"])
    assert queries > 100 and rays > 100 and paths > 30 and overlapped > 30


@pytest.mark.parametrize("flags", [0, NO_CULL])
@pytest.mark.parametrize("count", [0, COUNT])
@pytest.mark.parametrize("occluded", [0, OCCS[0]])
@pytest.mark.parametrize("tmax", [0, TMAXS[0]])
def test_footprint(tmax, occluded, count, flags):
    """Kernel 13 and exactly these rows in this order: the current generation read, the rays read, the limits read (only
    when given), the bytes written (only when given), the caller's counter added to atomically (only when given); no
    scratch, primary record, counter set, colour or accumulator.  Both outputs null: refused."""
    sc = OccScenario(120)
    try:
        if not occluded and not count:
            assert sc.L.rtc_plan_sim_occluded(sc.h, STREAM, RAYS[0], tmax, 0, 0, flags, sc.ops, 64, sc.fp, 256) == RTC_EINVAL
            return
        got = sc.occluded(STREAM, RAYS[0], tmax, occluded, count, flags)
        assert got["gen"] == 0
        want = [(R_GEN, READ, 0, 0, 1), (R_RAYS, READ, RAYS[0], 0, 1)]
        want += [(R_TMAX, READ, tmax, 0, 1)] if tmax else []
        want += [(R_OCC, WRITE, occluded, 0, 1)] if occluded else []
        want += [(R_SEG, ATOMIC, 0, 0, 1)] if count else []
        assert got["rows"] == want
        # a pipelined frame in flight (on a cull stream and the side stream) does not concern it: no wait either way
        sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        again = sc.occluded(STREAM, RAYS[1], tmax, occluded, count, flags)
        assert again["rows"][1] == (R_RAYS, READ, RAYS[1], 0, 1) and again["rows"][2:] == want[2:]
        assert sc.hazards() == []
    finally:
        sc.close()


def test_a_query_reads_the_generation_the_updates_made_current():
    sc = OccScenario(300)
    try:
        q = lambda: sc.occluded(STREAM, RAYS[0], TMAXS[0], OCCS[0], COUNT)  # noqa: E731
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
    """Not vacuous: an occlusion query moved to another stream without the order a caller owes (one stream at a time)
    races with the update that rewrites the generation it reads and with the query that writes the same bytes (the rays
    and limits are only read, and the counter is only added to: they race with nothing)."""
    sc = OccScenario(120)
    try:
        sc.update(STREAM)
        sc.occluded(STREAM, RAYS[0], TMAXS[0], OCCS[0], COUNT)
        sc.occluded(0x7f002000, RAYS[0], TMAXS[0], OCCS[0], COUNT, order_streams=False)
        sc.last_caller = ("caller", STREAM)  # (the update stays where the caller's order is)
        sc.update(STREAM)
        sc.update(STREAM)  # writes generation 1, which the stray query reads
        hz = sc.hazards(limit=50)
        assert {h[0] for h in hz} == {"occluded", "scene_gen"}, hz
        assert all("occluded" in (h[2][1], h[3][1]) for h in hz)
    finally:
        sc.close()


@pytest.mark.parametrize("what", ["no rays", "no output", "tile cull flag", "overlap flag", "unknown flag", "null sim"])
def test_refusals(what):
    """RTC_EINVAL where the entry point refuses; a refused query plans nothing and changes nothing."""
    sc = OccScenario(120)
    try:
        ok = dict(sim=sc.h, rays=RAYS[0], occluded=OCCS[0], count=COUNT, flags=0)
        bad = {"no rays": dict(rays=0), "no output": dict(occluded=0, count=0),
               "tile cull flag": dict(flags=rt.RTC_F_NO_TILE_CULL), "overlap flag": dict(flags=NO_CULL | OVERLAP),
               "unknown flag": dict(flags=0x8000), "null sim": dict(sim=None)}[what]
        a = dict(ok, **bad)
        assert sc.L.rtc_plan_sim_occluded(a["sim"], STREAM, a["rays"], TMAXS[0], a["occluded"], a["count"], a["flags"],
                                          sc.ops, 64, sc.fp, 256) == RTC_EINVAL
        sc.launch(_desc(64, 40, 4, 0, 1, 0, 0), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        assert "chain" in [k for k, _ in sc.kernel_order()]
        assert sc.occluded(STREAM, RAYS[0], 0, OCCS[0])["gen"] == 0
    finally:
        sc.close()
