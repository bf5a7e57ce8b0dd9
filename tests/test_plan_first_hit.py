"""The planner's side of the first-hit launch (rtc_render_first_hit_async; rtc_plan.h set_first_hit), on the
CPU through rtc_plan_sim_set_first_hit: a planned launch like any other -- it takes scratch slot 0's mask regions and
primary records, which pipelined launches in flight also own, so its waits come from plan_launch and tests/test_plan.py's
checker (vector clocks over the planned operations, unchanged) sees every byte it reads and writes.  Checked here: random
sequences that mix it with pipelined and joined launches, passes and scene updates are race free, and are not with the
legacy slot layout; what it runs and touches, and what it does not; a dropped wait is caught; the launches around it plan
as they did; its refusals.  No reference counterpart (main.c:263-304 renders frames only)."""
from __future__ import annotations

import ctypes as C
import random

import pytest

import raytracingc_amd as rt
from raytracingc_amd._abi import RTC_EINVAL
from test_plan import CAMS, ENVS, KERNEL, KNAMES as KN, OVERLAP, READ, RES_NAMES as RES, WAIT, WRITE, Scenario
from test_plan import _check_bound_regions, _desc, _random_launch
from test_plan_update import UpdateScenario

R_SCRATCH, R_PRIM, R_GEOSET, R_SAMPLES, R_COLORS, R_ACCUM = (RES.index(k) for k in
                                                             ("scratch", "prim", "geoset", "samples", "colors", "accum"))
R_GEN, R_HIT = RES.index("scene_gen"), RES.index("hit")
K_FIRST_HIT = KN.index("first_hit")
assert (R_HIT, K_FIRST_HIT) == (10, 10)
NO_CULL = rt.RTC_F_NO_TILE_CULL
STREAM = 0x7f001000
IDS = (0xA0000, 0xB0000, 0xC0000, 0xD0000)  # prim, depth, normal, albedo
SUPER_PIXELS = 400000  # rtc_plan.h kSuperCullPixels


class HitScenario(UpdateScenario):
    """test_plan_update.UpdateScenario (launches, passes through the sim, updates) plus first-hit launches, with this
    file's kernel and resource names."""

    def __init__(self, tri_count, legacy=False):
        Scenario.__init__(self, tri_count, legacy)
        self.stale, self.updates = set(), 0
        self.first_hits = set()  # launch numbers

    def first_hit(self, d, stream, ids, cam):
        assert self.L.rtc_plan_sim_set_first_hit(self.h, *ids) == 0
        self.first_hits.add(self.n)
        return self.launch(d, stream, 0x1000, 0x9000, True, cam, ENVS[0])  # (colours, accumulator, counters: ignored)

    def sample_pass(self, d, stream, colors, accum, rng, first, count, cam, env):
        assert self.L.rtc_plan_sim_set_sample_range(self.h, first, count, rng) == 0
        return self.launch(d, stream, colors, accum, False, cam, env)

    def rows_of(self, launch, kernel=None):
        """The footprint rows (resource, access, id, lo, hi) of one launch, of one of its kernels."""
        return [(a[1], a[2], a[3], a[4], a[5]) for a in self.accesses
                if a[7] == launch and (kernel is None or a[8] == kernel)]


def _kernels(sc):
    return [k for k, _ in sc.kernel_order()]


def _random_first_hit(rng, shape):
    """A first-hit launch of the shapes of test_plan._random_launch: whole frames and row / band shares, with and without
    RTC_F_NO_TILE_CULL, a random non-empty subset of the four buffers (two sets of identities)."""
    W, H = shape
    G = rng.choice([1, 1, 2, 4, 8])
    band = rng.choice([0, 0, 8]) if G > 1 else 0
    d = _desc(W, H, rng.choice([0, 1, 64]), rng.randrange(G) * (band or 1), G, band, NO_CULL if rng.random() < 0.3 else 0)
    d.trianglesOnly = rng.randrange(2)
    base = rng.choice([0, 0x100000])
    ids = [(i + base) if rng.random() < 0.6 else 0 for i in IDS]
    if not any(ids):
        ids[rng.randrange(4)] = IDS[0] + base
    return d, ids


def _sequences(seed, legacy=False, scenes=15, steps=24):
    """`scenes` scenes x `steps` steps: ordinary launches as tests/test_plan.py draws them (joined and RTC_F_OVERLAP, whole
    frames and row shares, three cameras), passes, updates and first-hit launches, on one or two caller streams.  Yields
    (scenario, first-hit launches below / above kSuperCullPixels, with / without the tile cull)."""
    rng = random.Random(9000 + seed)
    shapes = [(1920, 1080), (3840, 2160), (640, 360), (256, 256), (1000, 700)]
    for _ in range(scenes):
        sc = HitScenario(rng.choice([12, 120, 300, 5208]), legacy)
        if rng.random() < 0.33:
            assert sc.L.rtc_plan_sim_set_spheres(sc.h, rng.choice([1, 5, 40]), rng.randrange(2)) == 0
        streams = [rng.choice([0, 0x7f001000, 0x7f002000])]
        if rng.random() < 0.3:
            streams.append(rng.choice([0, 0x7f003000]))
        kinds = {"small": 0, "large": 0, "cull": 0, "brute": 0}
        try:
            shape = rng.choice(shapes)
            for _ in range(steps):
                st = rng.choice(streams)
                if rng.random() < 0.15:
                    sc.update(st)
                if rng.random() < 0.15:
                    shape = rng.choice(shapes)
                u = rng.random()
                if u < 0.3:
                    d, ids = _random_first_hit(rng, shape)
                    sc.first_hit(d, st, ids, rng.choice(CAMS))
                    kinds["large" if d.width * rt.lib().rtc_rows_selected(C.byref(d)) > SUPER_PIXELS else "small"] += 1
                    kinds["brute" if d.flags & NO_CULL else "cull"] += 1
                    continue
                d = _random_launch(rng, shape)
                if rng.random() < 0.5:
                    d.trianglesOnly = 0
                colors = rng.choice([0x1000, 0x2000, 0x3000])
                if u < 0.4:  # a pass of a progressive frame: joined, with its accumulator and states
                    d.flags &= ~OVERLAP
                    first = rng.randrange(d.spp)
                    sc.sample_pass(d, st, colors, 0x9000 + colors, 0xB000 + colors, first, rng.randint(1, d.spp - first),
                                   rng.choice(CAMS), rng.choice(ENVS))
                    continue
                seg = not (d.flags & OVERLAP) and rng.random() < 0.2
                sc.launch(d, st, colors, rng.choice([0, 0, 0, 0x9000 + colors]), seg, rng.choice(CAMS), rng.choice(ENVS))
            yield sc, kinds
        finally:
            sc.close()


@pytest.mark.parametrize("seed", range(20))
def test_random_sequences_with_first_hit_launches_are_race_free(seed):
    hits = 0
    for sc, kinds in _sequences(seed):
        hits += len(sc.first_hits)
        hz = sc.hazards()
        assert not hz, f"unordered conflicting kernels: {hz}"
        assert sc.n == 24
    assert hits > 50


def test_the_sequences_cover_both_sizes_and_both_paths():
    total = {"small": 0, "large": 0, "cull": 0, "brute": 0}
    for seed in range(3):
        for _, kinds in _sequences(seed):
            for k, v in kinds.items():
                total[k] += v
    assert all(v > 20 for v in total.values()), total


def test_legacy_slot_layout_races_in_the_same_sequences():
    """The checker sees the first-hit launches' scratch: with round 5's slot layout (slot h at h x the launch's own slot
    size) the same sequences have unordered scratch conflicts, and in some of them a first-hit launch's tile cull or
    rtc_first_hit is one of the two kernels (its slot 0 then overlaps another size's slot 1, which it does not wait
    for)."""
    seeds_with_hazard, involving_first_hit = 0, 0
    for seed in range(20):
        found = False
        for sc, _ in _sequences(seed, legacy=True):
            hz = sc.hazards(limit=200)
            found |= bool(hz)
            involving_first_hit += sum(1 for h in hz if h[0] == "scratch" and
                                       (h[2][0] in sc.first_hits or h[3][0] in sc.first_hits))
        seeds_with_hazard += found
    assert seeds_with_hazard >= 1, "the legacy slot layout must produce an unordered scratch conflict"
    assert involving_first_hit >= 1, "no conflict of the legacy layout involved a first-hit launch's scratch accesses"


@pytest.mark.parametrize("shape,share", [((640, 360), 1), ((1920, 1080), 1), ((1920, 1080), 4), ((3840, 2160), 8)])
@pytest.mark.parametrize("brute", [False, True])
@pytest.mark.parametrize("ids", [IDS, (IDS[0], 0, 0, 0), (0, 0, IDS[2], IDS[3])])
def test_footprint(shape, share, brute, ids):
    """What a first-hit launch runs and touches: {prep?, super_cull?, tile_cull, first_hit} on the caller's stream; the
    kernel reads its mask region (inside the bound regions), the slot's primary records and the scene generation, and
    writes one row per buffer asked for, with that buffer's identity; no colours, accumulator, counter set or sample
    slot; with RTC_F_NO_TILE_CULL no scratch row and no cull kernel."""
    W, H = shape
    sc = HitScenario(120)
    try:
        d = _desc(W, H, 0, share - 1, share, 0, NO_CULL if brute else 0)
        for cam, want_prep in ((CAMS[0], True), (CAMS[0], False), (CAMS[1], True)):
            info = sc.first_hit(d, STREAM, ids, cam)
            assert info == {"slot": 0, "alt": False, "overlap": False, "offset": 0}
            assert all(kind == KERNEL for kind, _, _, _ in sc.last_ops), "nothing in flight: no wait, and never a record"
            order = sc.kernel_order()
            assert {st for _, st in order} == {"caller"}
            large = W * ((H + share - 1) // share) > SUPER_PIXELS
            want = (["prep"] if want_prep else []) + (["super_cull"] if large and not brute else []) + \
                   ([] if brute else ["tile_cull"]) + ["first_hit"]
            assert [k for k, _ in order] == want
            rows = sc.rows_of(sc.n - 1, K_FIRST_HIT)
            res = [r[0] for r in rows]
            assert not {R_COLORS, R_ACCUM, R_GEOSET, R_SAMPLES} & {r[0] for r in sc.rows_of(sc.n - 1)}
            assert [(r[1], r[2]) for r in rows if r[0] == R_PRIM] == [(READ, 0)]
            assert [r[1] for r in rows if r[0] == R_GEN] == [READ]
            assert sorted((r[1], r[2]) for r in rows if r[0] == R_HIT) == sorted((WRITE, i) for i in ids if i)
            assert set(res) == {R_PRIM, R_GEN, R_HIT} | (set() if brute else {R_SCRATCH})
            if brute:
                assert not [r for r in sc.rows_of(sc.n - 1) if r[0] == R_SCRATCH] and sc.regions()["bound"] == {}
            else:
                g = _check_bound_regions(sc)
                assert set(g["bound"]) == {"mask", "pixMask", "weight"} | ({"superMask"} if large else set())
                mask = [(r[3], r[4]) for r in rows if r[0] == R_SCRATCH]
                assert mask == [g["bound"]["mask"]] and all(r[1] == READ for r in rows if r[0] == R_SCRATCH)
        assert sc.hazards() == []
    finally:
        sc.close()


def test_state_after_a_first_hit_launch_is_truthful():
    """Slot 0's primary records belong to the first-hit launch's camera origin afterwards: a render launch with another
    origin prepares again, one with the same origin (and a counter set the previous cull zeroed) does not; the first-hit
    launch itself reuses a render launch's records; an update makes them stale for it too."""
    sc = HitScenario(120)
    try:
        d = _desc(640, 360, 16, 0, 1, 0, 0)
        args = lambda cam: (d, STREAM, 0x1000, 0, False, cam, ENVS[0])  # noqa: E731
        sc.launch(*args(CAMS[0]))
        sc.launch(*args(CAMS[0]))
        assert "prep" not in _kernels(sc)
        sc.first_hit(d, STREAM, IDS, CAMS[0])
        assert _kernels(sc) == ["tile_cull", "first_hit"]  # (the render launch's records)
        sc.launch(*args(CAMS[0]))
        assert "prep" not in _kernels(sc), "the same origin: the records and the zeroed counter set are still good"
        sc.first_hit(d, STREAM, IDS, CAMS[1])
        assert _kernels(sc) == ["prep", "tile_cull", "first_hit"]
        sc.launch(*args(CAMS[0]))
        assert "prep" in _kernels(sc), "the first-hit launch left another origin's records in the slot"
        sc.update(STREAM)
        sc.first_hit(d, STREAM, IDS, CAMS[0])
        assert _kernels(sc)[0] == "prep" and not sc.prep_missing
        assert sc.rows_of(sc.n - 1, K_FIRST_HIT) and sc.generation_read() in (0, 1)
        assert sc.hazards() == []
    finally:
        sc.close()


def test_a_dropped_wait_is_caught():
    """An overlapped 1080p frame is in flight in slot 0 on a cull stream; the first-hit launch takes slot 0 on the caller's
    stream and its plan waits for that frame.  Replayed without the wait, its preparation and tile cull rewrite the
    records and masks the frame's geometry kernel reads: the checker reports it."""
    for drop in (False, True):
        sc = HitScenario(120)
        try:
            got = sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
            assert got["overlap"] and got["alt"] and got["slot"] == 0
            real_wait = sc.model.wait
            if drop:
                sc.model.wait = lambda st, ev: None
            sc.first_hit(_desc(1920, 1080, 0, 0, 1, 0, 0), STREAM, IDS, CAMS[1])
            sc.model.wait = real_wait
            waits = [(st, ev) for kind, st, ev, _ in sc.last_ops if kind == WAIT]
            assert waits == [(0, 3 + 0)], "the caller's stream waits for slot 0's sky-done event, and for nothing else"
            hz = sc.hazards(limit=50)
            if not drop:
                assert hz == []
            else:
                assert hz and all(1 in (h[2][0], h[3][0]) for h in hz), hz
                assert {h[0] for h in hz} >= {"scratch", "prim"}, hz
        finally:
            sc.close()


def test_it_waits_for_no_other_slot():
    """Frames in flight in slots 0 and 1: the first-hit launch waits for slot 0's alone (a render launch that is not
    overlapped waits for the newest)."""
    sc = HitScenario(120)
    try:
        for k in range(2):
            sc.launch(_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), STREAM, 0x1000 * (k + 1), 0, False, CAMS[0], ENVS[0])
        sc.first_hit(_desc(640, 360, 0, 0, 1, 0, 0), STREAM, IDS, CAMS[0])
        assert [(st, ev) for kind, st, ev, _ in sc.last_ops if kind == WAIT] == [(0, 3)]
        sc.first_hit(_desc(640, 360, 0, 0, 1, 0, 0), STREAM, IDS, CAMS[0])
        assert not [1 for kind, _, _, _ in sc.last_ops if kind == WAIT]  # (already waited for)
        assert sc.hazards() == []
    finally:
        sc.close()


# a fixed sequence of ordinary launches and passes: (desc, colours, accumulator, camera index, pass range or None)
_FIXED = [
    (_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), 0x1000, 0, 0, None),
    (_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), 0x2000, 0, 0, None),
    (_desc(1920, 1080, 64, 0, 1, 0, 0), 0x3000, 0, 0, None),
    (_desc(1920, 1080, 64, 0, 1, 0, 0), 0x3000, 0, 0, None),
    (_desc(640, 360, 16, 0, 1, 0, 0), 0x1000, 0xA000, 1, (0, 8)),
    (_desc(640, 360, 16, 0, 1, 0, 0), 0x1000, 0xA000, 1, (8, 8)),
    (_desc(1920, 1080, 64, 1, 4, 0, OVERLAP), 0x2000, 0, 1, None),
    (_desc(1920, 1080, 64, 2, 4, 0, OVERLAP), 0x2100, 0, 1, None),
    (_desc(256, 256, 1, 0, 1, 0, OVERLAP), 0x3000, 0, 0, None),
    (_desc(1000, 700, 16, 0, 1, 0, rt.RTC_F_NO_COOP), 0x1000, 0, 0, None),
    (_desc(1000, 700, 16, 0, 1, 0, rt.RTC_F_NO_COOP), 0x1000, 0, 0, None),
    (_desc(640, 360, 16, 0, 1, 0, NO_CULL), 0x1000, 0, 1, None),
    (_desc(1920, 1080, 64, 0, 1, 0, OVERLAP), 0x1000, 0, 0, None),
    (_desc(1920, 1080, 64, 0, 1, 0, 0), 0x2000, 0x9000, 1, None),
]


def _run_fixed(interleave):
    """The fixed sequence; with `interleave`, a first-hit launch after every launch of it: from the camera origin of
    CAMS[2], which no launch of the sequence uses, no larger than the 1080p frame the sequence starts with (so the scratch
    and its slot spacing grow when they did), alternately with and without the tile cull, 1080p and 640x360."""
    sc = HitScenario(300)
    out = []
    try:
        for i, (d, colors, accum, cam, rng) in enumerate(_FIXED):
            if rng:
                info = sc.sample_pass(d, STREAM, colors, accum, 0xB000, rng[0], rng[1], CAMS[cam], ENVS[0])
            else:
                info = sc.launch(d, STREAM, colors, accum, False, CAMS[cam], ENVS[0])
            out.append((info, sc.kernel_order(), sc.regions()["bound"]))
            if interleave:
                W, H = ((1920, 1080), (640, 360))[i % 2]
                sc.first_hit(_desc(W, H, 0, 0, 1, 0, NO_CULL if i % 3 == 2 else 0), STREAM, IDS, CAMS[2])
        assert sc.hazards() == []
        return out
    finally:
        sc.close()


def test_other_launches_plan_as_before():
    """The rule: with first-hit launches interleaved, every ordinary launch and pass takes the slot, the streams and the
    scratch regions (offsets and sizes) it takes without them, and runs the same kernels on the same streams in the same
    order -- except that a launch in slot 0 may run rtc_prep_primary where it did not, because the first-hit launch before
    it left slot 0's primary records at another camera origin.  Nothing else is added and nothing is dropped; a launch
    in another slot is unchanged altogether.  (Waits are not compared: a first-hit launch that waited for slot 0's frame
    spares a later launch that wait.)"""
    plain, mixed = _run_fixed(False), _run_fixed(True)
    assert len(plain) == len(mixed) == len(_FIXED)
    added = 0
    for i, ((info0, ks0, bound0), (info1, ks1, bound1)) in enumerate(zip(plain, mixed)):
        assert info0 == info1 and bound0 == bound1, (i, info0, info1, bound0, bound1)
        if ks0 != ks1:
            assert info0["slot"] == 0 and "prep" not in [k for k, _ in ks0], (i, ks0, ks1)
            assert [k for k in ks1 if k[0] != "prep"] == ks0 and [k for k, _ in ks1].count("prep") == 1, (i, ks0, ks1)
            added += 1
    assert added >= 2  # (the joined frame repeated with one camera, the second pass, the repeated one-lane launch)


@pytest.mark.parametrize("what", ["no buffer", "overlap", "no coop", "width", "stride", "band", "too large"])
def test_refusals(what):
    """RTC_EINVAL where the entry point refuses: every identity 0, a flag other than RTC_F_NO_TILE_CULL, bad geometry.
    The refused launch consumes the request: the next launch is an ordinary one."""
    d = {"no buffer": _desc(64, 40, 0, 0, 1, 0, 0), "overlap": _desc(64, 40, 0, 0, 1, 0, OVERLAP),
         "no coop": _desc(64, 40, 0, 0, 1, 0, rt.RTC_F_NO_COOP | NO_CULL), "width": _desc(0, 40, 0, 0, 1, 0, 0),
         "stride": _desc(64, 40, 0, 0, 0, 0, 0), "band": _desc(64, 40, 0, 0, 2, 3, 0),
         "too large": _desc(1 << 15, 1 << 15, 0, 0, 1, 0, 0)}[what]
    ids = (0, 0, 0, 0) if what == "no buffer" else IDS
    sc = HitScenario(120)
    try:
        L = sc.L
        assert L.rtc_plan_sim_set_first_hit(sc.h, *ids) == 0
        cam, env = (C.c_float * 13)(*CAMS[0]), (C.c_float * 14)(*ENVS[0])
        assert L.rtc_plan_sim_launch(sc.h, C.byref(d), STREAM, 0x1000, 0, 0, cam, env, sc.ops, 64, sc.fp, 256) == RTC_EINVAL
        sc.launch(_desc(64, 40, 4, 0, 1, 0, 0), STREAM, 0x1000, 0, False, CAMS[0], ENVS[0])
        assert "first_hit" not in _kernels(sc) and "chain" in _kernels(sc)
        assert L.rtc_plan_sim_set_first_hit(None, *IDS) == RTC_EINVAL
    finally:
        sc.close()


def test_no_rows_selected_plans_nothing():
    sc = HitScenario(120)
    try:
        sc.first_hit(_desc(64, 40, 0, 40, 1, 0, 0), STREAM, IDS, CAMS[0])
        assert sc.last_ops == [], "no kernel, and the caller's hooks stay armed: no record"
    finally:
        sc.close()
