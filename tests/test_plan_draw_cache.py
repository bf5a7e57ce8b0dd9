"""The launch planner with the draw cache on (rtc_plan.h Plan::draws; rtc_plan_sim_set_draw_cache), on tests/test_plan.py's
model of HIP streams and events: the launches that use the cache declare the slot table with its pool counter (resource 12:
written by the tile cull, ordered from cull to cull) and their slot's item-draw array (resource 13: written by the tile
cull, read by the geometry kernel), and a launch that clears the cache -- the first one, or one of another frame size --
or regrows the item-draw arrays reports a device synchronisation.  The pool's blocks are append-only and in no footprint.
The plans without the cache are tests/test_plan.py's, which runs unchanged.  Reference seam: main.c:263-304."""
from __future__ import annotations

from unittest import mock

import pytest

import raytracingc_amd as rt
import test_plan as tp

RES_DRAW_TABLE, RES_ITEM_DRAW = 12, 13
assert (tp.RES_NAMES[RES_DRAW_TABLE], tp.RES_NAMES[RES_ITEM_DRAW]) == ("draw_table", "item_draw")
NO_DRAW_CACHE = rt.RTC_F_NO_DRAW_CACHE
ARGS = (0x7f001000, 0x1000, 0, False, tp.CAMS[0], tp.ENVS[0])


class CachedScenario(tp.Scenario):
    """tests/test_plan.py's Scenario on a scene whose draw cache is on; counts the device synchronisations reported."""

    def __init__(self, tri_count, legacy=False):
        super().__init__(tri_count, legacy)
        assert self.L.rtc_plan_sim_set_draw_cache(self.h, 1) == 0
        self.syncs = 0
        sync = self.model.device_sync

        def counted():
            self.syncs += 1
            sync()

        self.model.device_sync = counted

    def rows(self, res):
        """The last launch's footprint rows on `res`: (kernel name, access, id)."""
        return [(tp.KNAMES[a[8]], a[2], a[3]) for a in self.accesses if a[7] == self.n - 1 and a[1] == res]


@pytest.mark.parametrize("seed", range(6))
def test_random_launch_sequences_are_race_free_with_the_cache(seed):
    """tests/test_plan.py's random sequences on scenes with the cache on: no unordered pair of conflicting kernels, the two
    new resources included -- and they do occur."""
    seen = {RES_DRAW_TABLE: 0, RES_ITEM_DRAW: 0}
    total = 0
    with mock.patch.object(tp, "Scenario", CachedScenario):
        for sc in tp._random_sequences(seed):
            total += sc.n
            hz = sc.hazards()
            assert not hz, f"unordered conflicting kernels: {hz}"
            for a in sc.accesses:
                if a[1] in seen:
                    seen[a[1]] += 1
    assert total == 50 * 24
    assert seen[RES_DRAW_TABLE] > 200 and seen[RES_ITEM_DRAW] > 2 * seen[RES_DRAW_TABLE] - 10, seen


def test_footprints_of_a_cached_launch():
    """A pipelined whole frame: the tile cull writes the table and the slot's item-draw array, the geometry kernel reads the
    array of the same slot; slot after slot.  The launches that never use the cache declare neither."""
    sc = CachedScenario(120)
    try:
        for k in range(3):
            got = sc.launch(tp._desc(1920, 1080, 64, 0, 1, 0, tp.OVERLAP), *ARGS)
            assert sc.rows(RES_DRAW_TABLE) == [("tile_cull", tp.WRITE, 0)]
            assert sc.rows(RES_ITEM_DRAW) == [("tile_cull", tp.WRITE, got["slot"]), ("chain", tp.READ, got["slot"])]
            assert got["slot"] == k
        for flags, segments in ((tp.OVERLAP | NO_DRAW_CACHE, False), (tp.OVERLAP | rt.RTC_F_HOIST_PRIMARY, False), (0, False),
                                (tp.CHAIN_INLINE, True), (rt.RTC_F_NO_TILE_CULL, False), (rt.RTC_F_DEBUG_BOUNCES, False)):
            sc.launch(tp._desc(1920, 1080, 64, 0, 1, 0, flags), 0x7f001000, 0x1000, 0, segments, tp.CAMS[0], tp.ENVS[0])
            assert sc.rows(RES_DRAW_TABLE) == [] and sc.rows(RES_ITEM_DRAW) == [], flags
        # a joined launch that sums in-kernel and a small share do
        sc.launch(tp._desc(1920, 1080, 64, 0, 1, 0, tp.CHAIN_INLINE), *ARGS)
        assert sc.rows(RES_DRAW_TABLE) and sc.rows(RES_ITEM_DRAW)
        sc.launch(tp._desc(1920, 1080, 64, 3, 8, 0, tp.OVERLAP), *ARGS)
        assert sc.rows(RES_DRAW_TABLE) and sc.rows(RES_ITEM_DRAW)
        # a sphere launch never does
        assert sc.L.rtc_plan_sim_set_spheres(sc.h, 5, 1) == 0
        with_spheres = tp._desc(1920, 1080, 64, 0, 1, 0, tp.OVERLAP)
        with_spheres.trianglesOnly = 0
        sc.launch(with_spheres, *ARGS)
        assert "chain" in [k for k, _ in sc.kernel_order()] and sc.rows(RES_DRAW_TABLE) == []
        assert sc.hazards() == []
    finally:
        sc.close()


def test_a_size_change_reports_a_synchronisation():
    """The first cached launch synchronises (the cache is allocated and cleared), the next ones of that frame size do not, a
    launch of another width or height does (the table is cleared; here the scratch does not grow: the frame is smaller),
    and so does the way back; a launch without the cache in between changes nothing."""
    sc = CachedScenario(120)
    try:
        def launch(w, h, flags=tp.OVERLAP):
            before = sc.syncs
            sc.launch(tp._desc(w, h, 64, 0, 1, 0, flags), *ARGS)
            return sc.syncs - before

        assert launch(1920, 1080) == 1
        assert [launch(1920, 1080) for _ in range(9)] == [0] * 9
        assert launch(1920, 1000) == 1  # the height alone
        assert launch(1920, 1000) == 0
        assert launch(1280, 1000) == 1
        assert launch(1920, 1080, tp.OVERLAP | NO_DRAW_CACHE) == 0
        assert launch(1280, 1000) == 0
        assert launch(1920, 1080) == 1
        # a row share of the same frame keeps the table: its seeds are frame rows
        sc.launch(tp._desc(1920, 1080, 64, 3, 8, 0, tp.OVERLAP), *ARGS)
        assert sc.rows(RES_DRAW_TABLE) and launch(1920, 1080) == 0
        assert sc.hazards() == []
    finally:
        sc.close()


def test_checker_sees_the_table_when_culls_are_unordered():
    """Not vacuous: two cached launches whose culls run on different streams, the second planned by a model that waits for
    nothing, race on the slot table."""
    sc = CachedScenario(120)
    try:
        sc.launch(tp._desc(1920, 1080, 64, 0, 8, 0, 0), 0, 0x1000, 0, False, tp.CAMS[0], tp.ENVS[0])
        real_wait = sc.model.wait
        sc.model.wait = lambda st, ev: None
        sc.launch(tp._desc(1920, 1080, 64, 1, 8, 0, tp.OVERLAP), 0x7f001000, 0x2000, 0, False, tp.CAMS[1], tp.ENVS[0])
        sc.model.wait = real_wait
        assert any(h[0] == "draw_table" for h in sc.hazards(limit=1000)), sc.hazards(limit=1000)
    finally:
        sc.close()
