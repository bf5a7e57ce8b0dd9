"""The launch planner with scene updates (rtc_plan.h plan_update; rtc_scene_update_async): the scene keeps two generations
of its records, a launch reads the current one, an update writes the other on the caller's stream and makes it current.
tests/test_plan.py's checker (vector clocks over the planned operations, no GPU) runs the same kind of random launch
sequences with an update before three steps in ten and the generations among the resources: no update may write records
a launch in flight reads, no launch may read records before their update wrote them, and every launch after an update
must derive its primary records again (they depend on the triangles, not only on the camera origin).  The steady
pipelined sequence pins what the two generations buy: an update never waits for the frame just enqueued.  The three
deliberate faults of rtc_plan_sim_set_update_fault show the checks are not vacuous.  No reference counterpart
(main.c:229-243 builds its arrays once, before the render loop)."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

from test_plan import CAMS, ENVS, KERNEL, KNAMES as KN, OVERLAP, RES_NAMES as RES, WAIT, Scenario, _desc, _random_launch

RES_SCENE_GEN = RES.index("scene_gen")
K_REFIT = KN.index("refit")
EV_SKY_DONE0, EV_GEO_DONE0, SLOTS = 3, 3 + 8, 8


class UpdateScenario(Scenario):
    """test_plan.Scenario plus rtc_plan_sim_update, and the bookkeeping of which slots' primary records an update made
    stale."""

    def __init__(self, tri_count, fault=0):
        super().__init__(tri_count)
        assert self.L.rtc_plan_sim_set_update_fault(self.h, fault) == 0
        self.stale = set()
        self.updates = 0

    def update(self, stream):
        caller = ("caller", stream)
        if self.last_caller is not None and self.last_caller != caller:  # (as Scenario.launch: one stream at a time)
            self.model.record(self.last_caller, ("caller-switch-u", self.n, self.updates))
            self.model.wait(caller, ("caller-switch-u", self.n, self.updates))
        self.last_caller = caller
        rc = self.L.rtc_plan_sim_update(self.h, stream, self.ops, 64, self.fp, 256)
        assert rc > 0, rc
        nops, nfp = rc & 0xFF, rc >> 8
        fps = np.frombuffer(self.fp, dtype=np.uint64, count=6 * nfp).reshape(nfp, 6).copy()
        assert fps[-1][0] == np.uint64(2**64 - 1)
        ops = [tuple(int(v) for v in self.ops[4 * i: 4 * i + 4]) for i in range(nops)]
        assert [o[0] for o in ops].count(KERNEL) == 1 and ops[-1][0] == KERNEL and ops[-1][3] == K_REFIT
        assert all(st == 0 for _, st, _, _ in ops), "an update runs on the caller's stream alone"
        for kind, _, ev, _ in ops[:-1]:
            assert kind == WAIT
            self.model.wait(caller, ("scene", ev))
        o = self.model.run(caller)
        for row in fps[:-1]:
            i, res, acc, ident, lo, hi = (int(v) for v in row)
            assert i == nops - 1 and res == RES_SCENE_GEN
            self.accesses.append((o, res, acc, ident, lo, hi, ("update", self.updates), self.n, K_REFIT))
        self.updates += 1
        self.stale = set(range(SLOTS))
        self.last_update_ops = ops
        return {"writes": int(fps[-1][2]), "waits": [ev for kind, _, ev, _ in ops if kind == WAIT]}

    def launch(self, *a, **kw):
        got = super().launch(*a, **kw)
        ks = [k for k, _ in self.kernel_order()]
        self.prep_missing = got["slot"] in self.stale and "prep" not in ks
        self.stale.discard(got["slot"])
        return got

    def generation_read(self):
        """The generation the last launch's kernels read (every kernel that reads one names the same)."""
        ids = {a[3] for a in self.accesses if a[7] == self.n - 1 and a[1] == RES_SCENE_GEN and a[8] != K_REFIT}
        assert len(ids) == 1, ids
        return ids.pop()


def _sequences(seed, fault=0):
    """50 scenes x 24 steps as tests/test_plan.py draws them, an update before a step with probability 0.3, caller stream
    switches, and spheres (gate open or shut) on a third of the scenes.  Yields (scenario, launches that lacked a
    preparation they needed)."""
    rng = random.Random(5000 + seed)
    shapes = [(1920, 1080), (3840, 2160), (640, 360), (256, 256), (1000, 700)]
    for _ in range(50):
        sc = UpdateScenario(rng.choice([12, 120, 300, 5208]), fault)
        if rng.random() < 0.33:
            assert sc.L.rtc_plan_sim_set_spheres(sc.h, rng.choice([1, 5, 40]), rng.randrange(2)) == 0
        streams = [rng.choice([0, 0x7f001000, 0x7f002000])]
        if rng.random() < 0.3:
            streams.append(rng.choice([0, 0x7f003000]))
        missing = 0
        try:
            shape = rng.choice(shapes)
            for _ in range(24):
                st = rng.choice(streams)
                if rng.random() < 0.3:
                    sc.update(st)
                if rng.random() < 0.15:
                    shape = rng.choice(shapes)
                d = _random_launch(rng, shape)
                if rng.random() < 0.5:
                    d.trianglesOnly = 0  # (render the spheres, where the scene has some)
                seg = not (d.flags & OVERLAP) and rng.random() < 0.2
                colors = rng.choice([0x1000, 0x2000, 0x3000])
                accum = rng.choice([0, 0, 0, 0x9000 + colors])
                sc.launch(d, st, colors, accum, seg, rng.choice(CAMS), rng.choice(ENVS))
                missing += sc.prep_missing
            yield sc, missing
        finally:
            sc.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_sequences_with_updates_are_race_free(seed):
    total = updates = 0
    for sc, missing in _sequences(seed):
        total += sc.n
        updates += sc.updates
        hz = sc.hazards()
        assert not hz, f"unordered conflicting kernels: {hz}"
        assert missing == 0, "a launch after an update kept primary records of the old triangles"
    assert total == 50 * 24 and updates > 200


def test_same_camera_after_update_prepares_again():
    """One camera, one stream: the second frame skips rtc_prep_primary, the frame after an update runs it, and reads the
    other generation."""
    sc = UpdateScenario(120)
    try:
        for flags in (0, OVERLAP):
            d = _desc(640, 360, 16, 0, 1, 0, flags)
            args = (d, 0x7f001000, 0x1000, 0, False, CAMS[0], ENVS[0])
            sc.launch(*args)
            sc.launch(*args)
            if not flags:  # (an overlapped launch takes the next slot, whose records it has to prepare anyway)
                assert "prep" not in [k for k, _ in sc.kernel_order()]
            g0 = sc.generation_read()
            up = sc.update(0x7f001000)
            assert up["writes"] == 1 - g0
            sc.launch(*args)
            assert "prep" in [k for k, _ in sc.kernel_order()] and not sc.prep_missing
            assert sc.generation_read() == 1 - g0
        assert sc.hazards() == []
    finally:
        sc.close()


def test_steady_pipelined_updates_keep_the_overlap():
    """Overlapped whole 1080p frames (the alternating cull streams), an update before each: update k waits for the slot of
    frame k - 2 -- the last reader of the generation it rewrites -- and for nothing else, never for frame k - 1, whose
    kernels are still running.  A second update with no frame between them rewrites the generation frame k - 1 reads and
    must wait for it; a third finds nothing pending."""
    sc = UpdateScenario(120)
    try:
        d = _desc(1920, 1080, 64, 0, 1, 0, OVERLAP)
        slots = []
        for k in range(20):
            up = sc.update(0x7f001000)
            want = [EV_SKY_DONE0 + slots[k - 2]] if k >= 2 else []
            assert up["waits"] == want, (k, up, slots)
            if k >= 1:
                assert not {EV_SKY_DONE0 + slots[-1], EV_GEO_DONE0 + slots[-1]} & set(up["waits"])
            got = sc.launch(d, 0x7f001000, 0x1000 + 0x1000 * (k % 3), 0, False, CAMS[0], ENVS[0])
            assert got["overlap"] and got["alt"]
            assert sc.generation_read() == up["writes"]
            slots.append(got["slot"])
        assert slots[:10] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
        assert sc.update(0x7f001000)["waits"] == [EV_SKY_DONE0 + slots[-2]]
        assert sc.update(0x7f001000)["waits"] == [EV_SKY_DONE0 + slots[-1]]
        assert sc.update(0x7f001000)["waits"] == []
        assert sc.hazards() == []
    finally:
        sc.close()


@pytest.mark.parametrize("fault", [1, 2, 3])
def test_checker_catches_broken_updates(fault):
    """rtc_plan_sim_set_update_fault: without the update's waits (1) or with the update writing the generation in use (3)
    some sequence has the refit kernel writing records a launch reads, unordered; with the primary records left valid (2)
    some launch after an update skips its preparation."""
    hazards = missing = 0
    for seed in range(6):
        for sc, m in _sequences(seed, fault):
            missing += m
            hz = sc.hazards()
            hazards += len(hz)
            assert all(h[0] == "scene_gen" for h in hz), hz
    if fault == 2:
        assert missing > 0 and hazards == 0
    else:
        assert hazards > 0, "the broken update must race a launch's reads of the scene records"
