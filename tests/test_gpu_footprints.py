"""Every byte a launch changes in the scene's memory lies where its own plan declares a write.

The method is snapshots, never fills: each span of DeviceScene.spans() is copied out (rtc_copy_async into a tensor of the
test's), the case is enqueued and the device synchronised, the spans are copied out again and the two snapshots diffed
against the write rows of DeviceScene.last_plan() -- the plan the executor ran (tests/footprints.py: allowed_ranges,
violations).  The test writes nothing into the scene's memory, so the kernels read what they would read anyway.  A diff
cannot see a byte rewritten with its old value: every case runs twice, each time behind different dirtying launches in the
same slot (another camera: at another frame size, then at the case's own, whose regions lie at the same offsets), and
what the two runs changed is united before the table of what a case must show written (Case.must) is asked.  (The
overlapped cases are not dirtied: an overlapped launch takes the next slot each time, so their runs land in slots nothing
has written yet or a launch of another shape wrote.)  The caller's buffers lie inside larger guard-filled tensors -- Color at an odd
byte offset, floats and words at a 4-byte offset that is not a multiple of 16 -- and every guard byte must survive.
Values are not compared here: the rest of the suite does that.  No reference counterpart (the scratch, its slots and the
plan are this project's)."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

import footprints as fpt
import raytracingc_amd as rt
from raytracingc_amd import _abi

pytestmark = pytest.mark.gpu

GUARD = 0xA5
CACHE_BLOCKS = 4096  # "a few thousand blocks": the pool is min(this, the frame's pixels) KB
WRITTEN: dict = {}   # case name -> what it showed written (test_the_matrix_as_a_whole_... runs what is not here yet)


class Guarded:
    """`nbytes` of a caller's buffer at `offset` bytes into a larger tensor filled with GUARD."""

    def __init__(self, nbytes, offset):
        import torch

        self.offset, self.nbytes = offset, nbytes
        self.t = torch.full((offset + nbytes + 256,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + offset

    def damage(self):
        """The guard bytes that changed, as offsets from the buffer's first byte (negative: before it; from nbytes on:
        behind it); empty when the guards are intact."""
        h = self.t.cpu().numpy()
        off = np.arange(len(h)) - self.offset
        return off[(h != GUARD) & ((off < 0) | (off >= self.nbytes))]

    def intact(self):
        return len(self.damage()) == 0

    def body(self):
        return self.t.cpu().numpy()[self.offset: self.offset + self.nbytes]


class Buffers:
    """The caller's buffers of a frame of up to `pixels` pixels: Color at an odd offset, the accumulator, the RNG states
    and the first-hit buffers at 4 mod 16, the five u64 segment counters at 8 mod 16."""

    def __init__(self, pixels):
        self.colors = Guarded(3 * pixels, 61)
        self.accum = Guarded(12 * pixels, 36)
        self.rng = Guarded(4 * pixels, 20)
        self.seg = Guarded(8 * rt.RTC_SEGMENT_COUNTERS, 40)
        self.hit = [Guarded(4 * pixels, 36), Guarded(4 * pixels, 52), Guarded(12 * pixels, 36), Guarded(12 * pixels, 20)]

    def all(self):
        return [self.colors, self.accum, self.rng, self.seg] + self.hit


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()  # (the whole device: an overlapped launch ends on the scene's own streams)


def snapshot(ds):
    """(spans, one uint8 array per span): rtc_copy_async wants 16-byte aligned addresses, so a span is copied from the
    16-byte boundary below its base (inside its allocation: hipMalloc's bases are aligned) and cut."""
    import torch

    _sync()
    spans = ds.spans()
    assert len(spans) == fpt.SPAN_COUNT
    held = []
    for _, _, _, base, nbytes in spans:
        base, nbytes = int(base), int(nbytes)
        if not nbytes:
            held.append(None)
            continue
        pre = base & 15
        t = torch.empty(pre + nbytes, dtype=torch.uint8, device="cuda")
        rt.copy_async(t.data_ptr(), base - pre, pre + nbytes, 32, _stream())
        held.append((t, pre))
    _sync()
    return spans, [np.zeros(0, np.uint8) if h is None else h[0].cpu().numpy()[h[1]:] for h in held]


def enqueue(ds, case, cam_args, bufs, size=None, kind=None, **more):
    cfg = case.config(size, **more)
    cam, scene = rt.camera_basis(*cam_args), rt.default_scene()
    kind = kind or case.kind
    seg = bufs.seg.ptr if case.segments and kind != "first_hit" else None
    if kind == "rows":
        ds.render_rows_async(scene, cam, cfg, bufs.colors.ptr, bufs.accum.ptr, seg, _stream())
    elif kind == "pass":
        ds.render_samples_async(scene, cam, cfg, case.first, case.count, bufs.colors.ptr, bufs.accum.ptr, bufs.rng.ptr, seg,
                                _stream())
    else:
        ds.render_first_hit_async(cam, cfg, *(h.ptr for h in bufs.hit), stream=_stream())


def checked(ds, what, enqueue_it, bufs=()):
    """Snapshot, enqueue, synchronise, snapshot: asserts (a) no changed byte outside the plan's writes and (b) the guards;
    returns (ops, rows, trailer, what showed written, the per-span diff)."""
    spans, before = snapshot(ds)
    enqueue_it()
    _sync()
    ops, rows, trailer = fpt.split_plan(*ds.last_plan())
    spans_after, after = snapshot(ds)
    assert np.array_equal(spans, spans_after), f"{what}: the launch reallocated a buffer (warm the scene up first)"
    diff = fpt.changed(before, after)
    allowed = fpt.allowed_ranges(rows, spans, fpt.pool_taken(spans, before, reset=bool(int(trailer[1]))))
    bad = fpt.violations(before, after, allowed, diff)
    described = [(fpt.SCENE_RES[int(spans[i][0])], int(spans[i][1]), int(spans[i][2]), off) for i, off in bad[:12]]
    assert not bad, f"{what}: {len(bad)} bytes changed outside the plan's writes, (resource, id, part, offset): {described}"
    for g in bufs:
        assert g.intact(), (f"{what}: guard bytes around a caller's buffer (at {g.offset} mod 16, {g.nbytes} bytes) changed, "
                            f"offsets from its first byte: {g.damage()[:16]} ({len(g.damage())} in all)")
    return ops, rows, trailer, fpt.written_names(ops, rows, spans, before, after, diff), diff


def upload(scene, cache):
    tris, sph, _ = fpt.geometry(scene)
    ds = rt.DeviceScene(tris, sph)
    ds.set_draw_cache(CACHE_BLOCKS if cache else 0)
    return ds


@pytest.fixture(scope="module")
def scenes(gpu_available):
    held = {}

    def get(scene, cache=False):
        if (scene, cache) not in held:
            held[(scene, cache)] = upload(scene, cache)
        return held[(scene, cache)]

    yield get
    _sync()
    for ds in held.values():
        ds.close()


def _dirty_sizes(case):
    w, h = case.size
    return (max(17, w - 7), max(2, h - 3)), (max(17, w - 19), max(2, h - 6))


def _dirty(ds, case, run, bufs):
    """Two joined launches in slot 0 from another camera, without the draw cache: one at another (smaller: nothing regrows)
    frame size, whose regions lie at other offsets, then one at the case's own size, which rewrites the very bytes of the
    case's regions, records and counters with another camera's values."""
    cfg = {k: v for k, v in case.cfg if k not in ("overlap", "row_stride")}
    plain = dataclasses.replace(case, cfg=tuple(cfg.items()), kind="rows", segments=False)
    for size in (_dirty_sizes(case)[run - 1], None):
        enqueue(ds, plain, case.camera_args()[run], bufs, size=size, draw_cache=False)
        for g in bufs.all():
            assert g.intact(), (f"{case.name}: a dirtying launch ({size or case.size}) changed guard bytes (buffer at "
                                f"{g.offset} mod 16, {g.nbytes} bytes): offsets {g.damage()[:16]} ({len(g.damage())} in all)")
    _sync()


def _prepare_cache(ds, case, run, bufs):
    """The draw cache's state before a cached case: filled from another camera and (cold) cleared again, so that what the
    case fills differs from what the blocks held."""
    if case.prepare in ("reset", "moved"):
        ds.draw_cache_reset()
        enqueue(ds, case, case.camera_args()[run], bufs)
        _sync()
    if case.prepare == "reset":
        ds.draw_cache_reset()
    if case.prepare == "same":
        enqueue(ds, case, case.camera_args()[0], bufs)
        _sync()


def run_case(ds, case):
    w, h = case.size
    bufs = Buffers(w * h)  # (the whole frame: the dirtying launches render every row of theirs, none larger)
    enqueue(ds, case, case.camera_args()[0], bufs)  # (warm-up: every buffer the case needs is allocated at its size)
    _sync()
    for g in bufs.all():
        assert g.intact(), (f"{case.name}: the first launch changed guard bytes (buffer at {g.offset} mod 16, {g.nbytes} "
                            f"bytes): offsets {g.damage()[:16]} ({len(g.damage())} in all)")
    if case.scene == "layers_33":  # (the issue's MULTI case: the geometry kernel ran over two chunks)
        rep = ds.chain_report()
        assert rep["multi"] and rep["chunk_count"] == 2, rep
    names, quiet = set(), True
    for run in (1, 2):
        _prepare_cache(ds, case, run, bufs)
        if "overlap" not in dict(case.cfg):
            _dirty(ds, case, run, bufs)
        ops, rows, trailer, wrote, diff = checked(
            ds, f"{case.name} run {run}", lambda: enqueue(ds, case, case.camera_args()[0], bufs), bufs.all())
        assert not set(case.absent) & set(fpt.kernels_of(ops)), fpt.kernels_of(ops)
        declared = {n for n, _, _ in fpt.scratch_write_rows(ops, rows)}
        assert {m for m in case.must if m in fpt.REGIONS} <= declared, (case.must, declared)
        names |= wrote
        quiet &= all(len(d) == 0 for d in diff)
    assert set(case.must) <= names, f"{case.name}: no changed byte seen in {set(case.must) - names} (seen: {sorted(names)})"
    if case.quiet:
        assert quiet, f"{case.name}: the launch changed the scene's memory"
    if case.kind != "first_hit":
        assert bufs.colors.body().any(), "the frame was written"
    WRITTEN[case.name] = names
    return names


SMALL = fpt.JOINED + [fpt.MERGE] + fpt.CACHED + fpt.PASSES + fpt.FIRST_HIT


def _small(name, scenes):
    case = next(c for c in SMALL if c.name == name)
    run_case(scenes(case.scene, case.cache), case)


def _large(name):
    case = next(c for c in fpt.LARGE if c.name == name)
    ds = upload(case.scene, False)
    try:
        run_case(ds, case)
        _sync()
    finally:
        ds.close()


@pytest.mark.parametrize("name", [c.name for c in SMALL])
def test_a_launch_writes_where_its_plan_says(name, scenes):
    _small(name, scenes)


@pytest.mark.parametrize("name", [c.name for c in fpt.LARGE])
def test_a_large_launch_writes_where_its_plan_says(name, gpu_available):
    """Above kSuperCullPixels, and wider than an item record's 16-bit coordinates: a scene of its own (its scratch is
    large, and every later snapshot would carry it)."""
    _large(name)


def test_nine_overlapped_launches_each_within_its_own_plan(gpu_available):
    """Every slot and both cull streams; the ninth launch takes the first one's slot again."""
    _overlapped()


def _overlapped():
    ds = upload("cube", False)
    try:
        bufs = Buffers(65 * 82)
        for case in fpt.OVERLAPPED[:2]:  # (joined warm-ups of both shapes: the scratch is at its size, slot 0 is next)
            joined = dataclasses.replace(case, cfg=tuple(kv for kv in case.cfg if kv[0] != "overlap"))
            enqueue(ds, joined, case.camera_args()[0], bufs)
        _sync()
        slots, streams, names = [], set(), set()
        for k, case in enumerate(fpt.OVERLAPPED):
            ops, rows, trailer, wrote, _ = checked(
                ds, case.name, lambda: enqueue(ds, case, case.camera_args()[k % 3], bufs), bufs.all())
            assert int(trailer[4]) == 1, "the launch was not overlapped"
            slots.append(int(trailer[2]))
            streams |= {int(o[1]) for o in ops if int(o[0]) == 0}
            assert set(case.must) <= wrote, (case.name, wrote)
            names |= wrote
        assert slots == [0, 1, 2, 3, 4, 5, 6, 7, 0] and streams == {0, 1, 2, 3}
        assert {"pixItem", "geoColor", "geoList", "prim", "geoset"} <= names
        WRITTEN["overlapped"] = names
    finally:
        _sync()
        ds.close()


def _device_tris(tris):
    import torch

    return torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).copy()).cuda()


def _moved(tris, dy):
    t = tris.copy()
    for k in ("posA", "posB", "posC"):
        t[k]["y"] += np.float32(dy)
    return t


def _generation_diffs(spans, diff):
    return {int(spans[i][1]) for i in range(len(spans)) if int(spans[i][0]) == fpt.RES_SCENE_GEN and len(diff[i])}


def test_an_update_writes_the_other_generation_and_a_regroup_the_membership(gpu_available):
    _update_regroup()


def _update_regroup():
    tris = fpt.geometry("fsuzane")[0]
    ds = upload("fsuzane", False)
    try:
        names = set()
        for step, dy in enumerate((0.25, -0.5)):  # generation 1, then generation 0
            dev = _device_tris(_moved(tris, dy))
            ops, rows, trailer, wrote, diff = checked(ds, f"update {step}", lambda: ds.update(dev, stream=_stream()))
            assert fpt.kernels_of(ops) == ["refit"] and int(trailer[2]) == 1 - step
            assert _generation_diffs(ds.spans(), diff) == {1 - step} and wrote == {"scene_gen"}
            names |= wrote
        # a regroup from the same triangles in another order: the membership is that of a fresh upload of them
        order = np.random.default_rng(5).permutation(len(tris))
        dev = _device_tris(tris[order])
        nbytes = ds.regroup_scratch_bytes()
        scratch = Guarded(nbytes, 64)
        ops, rows, trailer, wrote, diff = checked(
            ds, "regroup", lambda: ds.regroup_async(dev.data_ptr(), None, scratch.ptr, nbytes, _stream()), [scratch])
        assert fpt.kernels_of(ops)[0] == "regroup_centroids" and fpt.kernels_of(ops)[-2:] == ["regroup_index", "refit"]
        assert _generation_diffs(ds.spans(), diff) == {1} and wrote == {"scene_gen", "membership"}
        assert (scratch.body() != GUARD).any(), "the caller's scratch was used"
        WRITTEN["update_regroup"] = names | wrote
    finally:
        _sync()
        ds.close()


def test_an_update_between_overlapped_launches_leaves_the_bound_generation(gpu_available):
    """Launch, update, launch, enqueued without a synchronisation between them: the first launch's generation is
    byte-identical afterwards, and what changed lies in the three plans' writes."""
    tris = fpt.geometry("cube")[0]
    ds = upload("cube", False)
    try:
        case = fpt.OVERLAPPED[1]
        bufs, other = Buffers(65 * 82), Buffers(65 * 82)
        joined = dataclasses.replace(case, cfg=tuple(kv for kv in case.cfg if kv[0] != "overlap"))
        enqueue(ds, joined, case.camera_args()[0], bufs)
        _sync()
        dev = _device_tris(_moved(tris, 0.125))
        spans, before = snapshot(ds)
        plans = []
        enqueue(ds, case, case.camera_args()[0], bufs)
        plans.append(fpt.split_plan(*ds.last_plan()))
        ds.update(dev, stream=_stream())
        plans.append(fpt.split_plan(*ds.last_plan()))
        enqueue(ds, case, case.camera_args()[1], other)
        plans.append(fpt.split_plan(*ds.last_plan()))
        _sync()
        spans_after, after = snapshot(ds)
        assert np.array_equal(spans, spans_after)
        assert [fpt.kernels_of(p[0])[-1] for p in plans] == ["sky", "refit", "sky"] and int(plans[1][2][2]) == 1
        reads = [{int(r[3]) for r in p[1] if int(r[1]) == fpt.RES_SCENE_GEN and int(r[2]) == fpt.READ} for p in plans]
        assert reads[0] == {0} and reads[2] == {1}, "the launches bind the generation current when they were enqueued"
        allowed = {}
        for _, rows, _ in plans:
            for i, ranges in fpt.allowed_ranges(rows, spans).items():
                allowed.setdefault(i, []).extend(ranges)
        diff = fpt.changed(before, after)
        assert fpt.violations(before, after, allowed, diff) == []
        assert _generation_diffs(spans, diff) == {1}
        assert all(g.intact() for g in bufs.all() + other.all())
    finally:
        _sync()
        ds.close()


def _rays(n, seed):
    """n rays from the cube camera's origin towards the cube and past it (hits and misses)."""
    import torch

    rng = np.random.default_rng(seed)
    origin, at = np.float32(fpt.CUBE_CAMERAS[0][0]), np.float32(fpt.CUBE_CAMERAS[0][1])
    rays = np.zeros((n, 6), np.float32)
    rays[:, :3] = origin
    rays[:, 3:] = (at - origin) + rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    return torch.from_numpy(rays).cuda()


def test_the_queries_change_nothing_of_the_scenes(scenes):
    """rtc.h: a query uses no scratch, primary record, counter set, stream or event of the scene's -- every span is
    byte-identical behind each of them, and their outputs stay inside their buffers."""
    import torch

    ds = scenes("cube")
    n = 300  # (more than one workgroup of a lane per ray)
    rays = _rays(n, 11)
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    scene, cam = rt.default_scene(), rt.camera_basis(*fpt.CUBE_CAMERAS[0])
    hit = [Guarded(4 * n, 36), Guarded(4 * n, 52), Guarded(12 * n, 36), Guarded(12 * n, 20)]
    radiance, seeds_out, count = Guarded(12 * n, 36), Guarded(4 * n, 20), Guarded(8, 40)
    occluded, tmax = Guarded(n, 61), torch.full((n,), 100.0, dtype=torch.float32, device="cuda")
    cfg = rt.RenderConfig(64, 40, 4, 10, True)
    px = 64 * 40
    pixels = torch.from_numpy(np.random.default_rng(3).permutation(px)[:n].astype(np.int32)).cuda()
    colors, accum, rng = Guarded(3 * px, 61), Guarded(12 * px, 36), Guarded(4 * px, 20)
    order, keys = Guarded(4 * n, 36), Guarded(4 * n, 52)
    sort_bytes = rt.ray_order_scratch_bytes(n)
    sort_scratch = Guarded(sort_bytes, 64)
    st = _stream()
    queries = {
        "trace_rays": (lambda: ds.trace_rays_async(rays.data_ptr(), n, True, 0, *(h.ptr for h in hit), stream=st), hit),
        "trace_paths": (lambda: ds.trace_paths_async(scene, rays.data_ptr(), seeds.data_ptr(), n, 4, 10, radiance.ptr, True,
                                                     0, 0, None, seeds_out.ptr, count.ptr, st), [radiance, seeds_out, count]),
        "trace_paths_wave": (lambda: ds.trace_paths_async(scene, rays.data_ptr(), seeds.data_ptr(), n, 4, 10, radiance.ptr,
                                                          True, rt.RTC_F_WAVE_PER_RAY, 0, None, seeds_out.ptr, count.ptr, st),
                             [radiance, seeds_out, count]),
        "occluded": (lambda: ds.occluded_async(rays.data_ptr(), n, tmax.data_ptr(), True, 0, occluded.ptr, count.ptr, st),
                     [occluded, count]),
        "render_pixels": (lambda: ds.render_pixels_async(scene, cam, cfg, 0, 2, pixels.data_ptr(), n, accum.ptr, rng.ptr,
                                                         colors.ptr, count.ptr, 0, st), [colors, accum, rng, count]),
        "render_pixels_wave": (lambda: ds.render_pixels_async(scene, cam, cfg, 2, 2, pixels.data_ptr(), n, accum.ptr, rng.ptr,
                                                              colors.ptr, count.ptr, rt.RTC_F_WAVE_PER_RAY, st),
                               [colors, accum, rng, count]),
    }
    kernels = {"trace_paths_wave": "trace_paths", "render_pixels_wave": "render_pixels"}
    for name, (call, outs) in queries.items():
        ops, rows, trailer, wrote, diff = checked(ds, name, call, outs)
        assert fpt.kernels_of(ops) == [kernels.get(name, name)]
        assert all(len(d) == 0 for d in diff), f"{name} changed the scene's memory"
        assert all((g.body() != GUARD).any() for g in outs), f"{name} wrote its outputs"
    # the ray order plans nothing (it touches nothing of the scene's state): the record stays the last query's
    last = ds.last_plan()
    spans, before = snapshot(ds)
    ds.ray_order_async(rays.data_ptr(), n, order.ptr, sort_scratch.ptr, sort_bytes, None, keys.ptr, st)
    _sync()
    _, after = snapshot(ds)
    assert all(len(d) == 0 for d in fpt.changed(before, after)), "rtc_ray_order_async changed the scene's memory"
    assert all(g.intact() for g in (order, keys, sort_scratch)) and (order.body() != GUARD).any()
    assert all(np.array_equal(a, b) for a, b in zip(last, ds.last_plan()))


def test_the_spans_are_the_scenes_allocations(scenes):
    """Before its first launch a scene has its records, counters and membership and no scratch, samples or draw cache;
    the spans of one resource do not overlap, and the record before anything was enqueued is empty."""
    ds = upload("cube", True)
    try:
        ops, rows = ds.last_plan()
        assert len(ops) == 0 and len(rows) == 0
        L, raw_ops, raw_rows = rt.lib(), np.zeros((48, 4), np.int32), np.zeros((256, 6), np.uint64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert L.rtc_scene_last_plan(ds._h, ptr(raw_ops), 0, ptr(raw_rows), 0) == 0, "nothing enqueued yet: 0, whatever the room"
        few = np.zeros((fpt.SPAN_COUNT - 1, 5), np.uint64)
        assert L.rtc_scene_spans(ds._h, ptr(few), fpt.SPAN_COUNT - 1) == _abi.RTC_EINVAL
        assert b"rtc_scene_spans" in L.rtc_last_error()
        assert L.rtc_scene_spans(ds._h, ptr(few), 0) == _abi.RTC_EINVAL and L.rtc_scene_spans(ds._h, None, 64) == _abi.RTC_EINVAL
        spans = ds.spans()
        assert len(spans) == fpt.SPAN_COUNT
        empty = {fpt.SCENE_RES[int(s[0])] for s in spans if int(s[4]) == 0}
        assert empty == {"scratch", "samples", "draw_table", "item_draw", "draw_pool"}
        assert all(int(s[3]) == 0 for s in spans if int(s[4]) == 0)
        bufs = Buffers(64 * 40)
        # an empty launch (no row selected) records the planner's empty plan: the caller's two hooks, no kernel, no row
        none = dataclasses.replace(fpt.CACHED[0], cfg=fpt.CACHED[0].cfg + (("row_start", 40),))
        assert none.config().rows() == 0
        _, before = snapshot(ds)
        enqueue(ds, none, fpt.CUBE_CAMERAS[0], bufs)
        ops, rows, trailer = fpt.split_plan(*ds.last_plan())
        assert [tuple(int(v) for v in o) for o in ops] == [(1, 0, 20, -1), (1, 0, 19, -1)] and len(rows) == 0
        assert all(len(d) == 0 for d in fpt.changed(before, snapshot(ds)[1])) and all(g.intact() for g in bufs.all())
        enqueue(ds, fpt.CACHED[0], fpt.CUBE_CAMERAS[0], bufs)
        _sync()
        # outputs with less room than the plan has are refused, and nothing is copied
        ops, rows = ds.last_plan()
        assert len(ops) >= 4 and len(rows) >= 20
        raw_ops[:], raw_rows[:] = 7, 7
        for max_ops, max_rows in ((len(ops) - 1, 256), (48, len(rows) - 1), (0, 0)):
            assert L.rtc_scene_last_plan(ds._h, ptr(raw_ops), max_ops, ptr(raw_rows), max_rows) == _abi.RTC_EINVAL
            assert b"rtc_scene_last_plan" in L.rtc_last_error() and (raw_ops == 7).all() and (raw_rows == 7).all()
        assert L.rtc_scene_last_plan(ds._h, None, 48, ptr(raw_rows), 256) == _abi.RTC_EINVAL
        rc = L.rtc_scene_last_plan(ds._h, ptr(raw_ops), len(ops), ptr(raw_rows), len(rows))
        assert rc == len(ops) | len(rows) << 8 and np.array_equal(raw_ops[:len(ops)], ops) and np.array_equal(raw_rows[:len(rows)], rows)
        spans = ds.spans()
        assert {fpt.SCENE_RES[int(s[0])] for s in spans if int(s[4]) == 0} == {"samples"}
        pool = next(s for s in spans if int(s[0]) == fpt.RES_DRAW_POOL)
        assert int(pool[4]) == min(CACHE_BLOCKS, 64 * 40) * fpt.DRAW_BLOCK_BYTES
        live = sorted((int(s[3]), int(s[3]) + int(s[4])) for s in spans if int(s[4]))
        assert all(a[1] <= b[0] for a, b in zip(live, live[1:])), "two spans overlap"
        scratch = next(s for s in spans if int(s[0]) == fpt.RES_SCRATCH)
        assert int(scratch[4]) % fpt.SLOTS == 0
    finally:
        _sync()
        ds.close()


def test_the_matrix_as_a_whole_shows_every_region_and_resource_written(scenes):
    """Non-vacuity over the whole matrix: every region of the slot and every resource outside it showed a changed byte
    inside a declared write in some case (the segment slots excepted: the reduce kernel leaves them zero, as it found
    them).  The cases the tests above ran in this session are not run again; run alone, this test runs them all."""
    runs = {c.name: (lambda n=c.name: _small(n, scenes)) for c in SMALL}
    runs.update({c.name: (lambda n=c.name: _large(n)) for c in fpt.LARGE})
    runs.update(overlapped=_overlapped, update_regroup=_update_regroup)
    for name, run in runs.items():
        if name not in WRITTEN:
            run()
    seen = set().union(*(WRITTEN[name] for name in runs))
    assert seen >= fpt.WHOLE_MATRIX, fpt.WHOLE_MATRIX - seen
