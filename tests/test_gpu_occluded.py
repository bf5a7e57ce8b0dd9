"""rtc_occluded_async / rtc_occluded on the GPU (include/rtc.h): one byte per ray -- does
calculateRayCollision(ray, trianglesOnly) (raytracing.c:216-240) hit with dst < tMax -- and the launch's count, against the
CPU oracle (tests/occlusion_reference.py), compared exactly for every ray, under flags 0 and RTC_F_NO_CLUSTER_CULL.  The
sets' premises (a tie occludes nothing, one ulp above occludes every hit, the median splits the hits) are
tests/test_occlusion_reference.py's, without a GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import moving_scenes
import occlusion_reference as oc
import raytracingc_amd as rt
import trace_rays_reference as tr

pytestmark = pytest.mark.gpu

F = np.float32
FLAGS = oc.FLAGS
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def _scene(name):
    tris, spheres = tr.geometry(name)[:2]
    return rt.DeviceScene(tris, spheres)


def _dev(rays):
    """The rays as a float32 [n, 6] tensor on the device."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6).copy()).cuda()


def _check(ds, rays, lim, tonly, want, what):
    """Bytes and count under every flag against the expectation (bool [n]); returns the number of occluded rays."""
    d = _dev(rays)
    for flags in FLAGS:
        got, count = ds.occluded(d, lim, bool(tonly), flags, count=True)
        bad = int((got != want).sum())
        print(f"{what} flags {flags:#x}: {len(rays)} rays, {int(want.sum())} occluded, differing {bad}, count {count}")
        assert got.dtype == bool and got.shape == want.shape and bad == 0, f"{what} flags {flags:#x}"
        assert count == int(want.sum()), f"{what} flags {flags:#x}: the count"
    return int(want.sum())


@pytest.mark.parametrize("kind", ["primary", "replay"])
@pytest.mark.parametrize("name", sorted(tr.REPLAY))
def test_named_sets(name, kind, gpu_available):
    """The primary rays and the recorded bounce rays of every case under every limit set.  tie: no ray set (the unsigned
    tie trap: an accepted dst == L shows here); above: every hit set (a dropped ball or a lane retired too early shows
    here)."""
    tonly = tr.geometry(name)[2]
    hits = int((tr.case_expected(kind, name)["prim"] != -1).sum())
    for limit in oc.LIMITS:
        n = _check(_scene(name), tr.case_rays(kind, name), oc.case_limits(kind, name, limit), tonly,
                   oc.case_occluded(kind, name, limit), f"{kind} {name} {limit}")
        if limit == "tie":
            assert n == 0
        if limit == "above":
            assert n == hits and (kind != "replay" or n == tr.REPLAY[name][1])


@pytest.mark.parametrize("scale", tr.SCALES)
@pytest.mark.parametrize("name", tr.SCALED_CASES)
def test_scaled_sets(name, scale, gpu_available):
    """dir times 0.25, 3 (lanes beyond the bound's premise in waves whose other lanes cull), 1e-3 and 1e4, with the scaled
    rays' own above, median and short limits."""
    for limit in ("above", "median", "short"):
        _check(_scene(name), tr.scaled(name, scale), oc.case_limits("scaled", name, limit, scale), 1,
               oc.case_occluded("scaled", name, limit, scale), f"scaled {name} x{scale} {limit}")


@pytest.mark.parametrize("name", ["chunks", "default", "box_mirror"])
def test_segments(name, gpu_available):
    """Line of sight: pos = a, dir = b - a, tMax = 1, the segments ending on the surfaces the replay rays hit."""
    tris, spheres, tonly, _ = tr.geometry(name)
    rays, lim = oc.segments(name)
    _check(_scene(name), rays, lim, tonly, oc.expected(tris, spheres, tonly, rays, lim), f"segments {name}")


@pytest.mark.parametrize("tonly", [0, 1])
def test_odd_rays(tonly, gpu_available):
    """NaN, infinite, zero, tiny and huge components against the default scene, with and without its sphere."""
    tris, spheres, _, _ = tr.geometry("default")
    rays = tr.odd()[0]
    e = tr.case_expected("odd", "default", None, tonly)
    for limit in ("none", "odd"):
        lim = oc.limits(limit, e["prim"], e["depth"])
        _check(_scene("default"), rays, lim, tonly, oc.expected(tris, spheres, tonly, rays, lim), f"odd tonly {tonly} {limit}")


@pytest.mark.parametrize("name", tr.EXTRA)
def test_extra_scenes(name, gpu_available):
    """A scene without a triangle, 33 spheres, the tie scenes, the counts around a cluster and the layers around a chunk:
    the sphere loop and the chunk-level loop."""
    tonly = tr.geometry(name)[2]
    for limit in ("none", "tie", "above"):
        n = _check(_scene(name), tr.case_rays("extra", name), oc.case_limits("extra", name, limit), tonly,
                   oc.case_occluded("extra", name, limit), f"extra {name} {limit}")
        if limit == "tie":
            assert n == 0


def test_spheres_present_but_skipped(gpu_available):
    """trianglesOnly = 1 on the default scene's replay rays: the sphere is resident and must not occlude."""
    tris, spheres, _, _ = tr.geometry("default")
    rays = tr.replay("default")
    for limit in ("none", "above", "median"):
        lim = oc.case_limits("replay", "default", limit)  # from the closest hits WITH the sphere
        want = oc.expected(tris, spheres, 1, rays, lim)
        if limit == "above":  # one ulp past the sphere's surface: occluded by the sphere, not by the triangle behind it
            assert (want != oc.case_occluded("replay", "default", limit)).sum() >= tr.DEFAULT_SPHERE_HITS // 2
        _check(_scene("default"), rays, lim, 1, want, f"default trianglesOnly {limit}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097])
def test_ray_counts_and_guards(n, gpu_available):
    """The tail: a lone live lane in a wave, partial waves and blocks; the output at byte offsets 1, 2 and 3 in a
    guard-filled buffer: exactly bytes [0, n) are written, each 0 or 1; a counter preset to 5 ends at 5 + the set bytes;
    each output alone."""
    import torch

    base = tr.replay("chunks")
    reps = n // len(base) + 1
    rays = np.concatenate([base] * reps)[:n]
    lim = np.concatenate([oc.case_limits("replay", "chunks", "median")] * reps)[:n]
    want = np.concatenate([oc.case_occluded("replay", "chunks", "median")] * reps)[:n]
    ds, d, t = _scene("chunks"), _dev(rays), torch.from_numpy(lim.copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for flags in FLAGS:
        for off in (1, 2, 3):
            buf = torch.full((n + 8,), GUARD, dtype=torch.uint8, device="cuda")
            cnt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ds.occluded_async(d.data_ptr(), n, t.data_ptr(), True, flags, buf.data_ptr() + off, cnt.data_ptr(), stream=st)
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert (host[:off] == GUARD).all() and (host[off + n:] == GUARD).all(), "a byte outside [0, n) was written"
            assert np.isin(host[off:off + n], (0, 1)).all()
            assert np.array_equal(host[off:off + n].astype(bool), want), (flags, off)
            assert int(cnt.cpu().numpy()[0]) == 5 + int(want.sum())
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        buf = torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ds.occluded_async(d.data_ptr(), n, t.data_ptr(), True, flags, 0, cnt.data_ptr(), stream=st)  # the count alone
        ds.occluded_async(d.data_ptr(), n, t.data_ptr(), True, flags, buf.data_ptr(), 0, stream=st)  # the bytes alone
        torch.cuda.synchronize()
        assert int(cnt.cpu().numpy()[0]) == int(want.sum())
        assert np.array_equal(buf.cpu().numpy(), want.astype(np.uint8))


def test_permutation(gpu_available):
    """Permuting rays and limits together permutes the bytes: an early-exit wave does not let one lane's answer depend on
    its neighbours."""
    parts = [("replay", "chunks", None), ("scaled", "chunks", 3.0), ("primary", "chunks", None)]
    rays = np.concatenate([tr.case_rays(k, n, s) for k, n, s in parts])
    for limit in ("median", "short", "above"):
        lim = np.concatenate([oc.case_limits(k, n, limit, s) for k, n, s in parts])
        want = np.concatenate([oc.case_occluded(k, n, limit, s) for k, n, s in parts])
        perm = np.random.default_rng(11).permutation(len(rays))
        _check(_scene("chunks"), rays[perm], lim[perm], 1, want[perm], f"permuted {limit}")


@pytest.mark.parametrize("name", ["chunks", "mixed_scale", "default"])
def test_mixed_waves(name, gpu_available):
    """Lane by lane within one launch: a NaN limit (never seeking), short, inf, and a ray that misses everything.  The wave
    leaves only when its last seeker is done."""
    tris, spheres, tonly, _ = tr.geometry(name)
    base, e = tr.replay(name), tr.case_expected("replay", name)
    short = oc.case_limits("replay", name, "short")
    miss = np.flatnonzero(e["prim"] == -1)
    hit = np.flatnonzero(e["prim"] != -1)
    assert len(miss) >= 1 and len(hit) >= 64
    n = len(hit) // 4 * 4
    rays, lim = base[hit[:n]].copy(), np.zeros(n, F)
    lim[0::4], lim[1::4], lim[2::4], lim[3::4] = np.nan, short[hit[:n]][1::4], np.inf, np.inf
    rays[3::4] = base[miss[np.arange(n // 4) % len(miss)]]
    want = oc.expected(tris, spheres, tonly, rays, lim)
    assert not want[0::4].any() and want[2::4].all() and not want[3::4].any()
    _check(_scene(name), rays, lim, tonly, want, f"mixed {name}")
    # one seeker (a ray that hits) among 63 lanes that never seek
    lone = np.full(n, np.nan, F)
    lone[6::64] = np.inf
    want = oc.expected(tris, spheres, tonly, rays, lone)
    assert want.sum() >= 1
    _check(_scene(name), rays, lone, tonly, want, f"lone seeker {name}")


def test_after_a_scene_update(gpu_available):
    """A query enqueued before DeviceScene.update on the same stream sees the old triangles, one enqueued after it the new
    ones, and the two differ: the balls are refit, and the cull follows them."""
    import torch

    tris = tr.geometry("chunks")[0]
    moved = moving_scenes.HELPERS["shift"](tris)
    rays = np.concatenate([tr.replay("chunks"), tr.primary("chunks")])
    e0, e1 = tr.expected(tris, None, 1, rays), tr.expected(moved, None, 1, rays)
    n, d = len(rays), _dev(rays)
    ds = rt.DeviceScene(tris, None)
    try:
        for limit in ("median", "above"):
            lim = oc.limits(limit, e0["prim"], e0["depth"])
            before, after = oc.expected(tris, None, 1, rays, lim), oc.expected(moved, None, 1, rays, lim)
            assert (before != after).sum() > 20, "the move must show"
            for flags in FLAGS:
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    dev_tris = [torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).copy()).cuda() for t in (moved, tris)]
                    t = torch.from_numpy(lim.copy()).cuda()
                    old = torch.zeros(n, dtype=torch.uint8, device="cuda")
                    new = torch.zeros(n, dtype=torch.uint8, device="cuda")
                    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
                    st.synchronize()
                    ds.occluded_async(d.data_ptr(), n, t.data_ptr(), True, flags, old.data_ptr(), cnt.data_ptr(),
                                      stream=st.cuda_stream)
                    ds.update(tris=dev_tris[0], stream=st.cuda_stream)
                    ds.occluded_async(d.data_ptr(), n, t.data_ptr(), True, flags, new.data_ptr(), cnt.data_ptr() + 8,
                                      stream=st.cuda_stream)
                    st.synchronize()
                    assert np.array_equal(old.cpu().numpy().astype(bool), before), "the query before the update saw the new triangles"
                    assert np.array_equal(new.cpu().numpy().astype(bool), after), (limit, flags)
                    assert list(cnt.cpu().numpy()) == [int(before.sum()), int(after.sum())]
                    ds.update(tris=dev_tris[1], stream=st.cuda_stream)  # back, for the next flag
                    st.synchronize()
    finally:
        torch.cuda.synchronize()
        ds.close()


def _frame(ds, scene, cam, cfg, st, event=False):
    import torch

    rows = cfg.rows()
    col = torch.zeros((rows, cfg.width, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((rows, cfg.width, 3), dtype=torch.float32, device="cuda")
    st.synchronize()
    ev = None
    if event:
        ev = torch.cuda.Event()
        ev.record(st)  # (a torch event has no hipEvent_t before its first record)
        ds.set_frame_event(ev.cuda_event)
    ds.render_rows_async(scene, cam, cfg, col.data_ptr(), acc.data_ptr(), None, st.cuda_stream)
    return col, acc, ev


def _same(a, b):
    return all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in zip(a[:2], b[:2]))


def test_between_frames_and_passes(gpu_available):
    """Queries between pipelined (RTC_F_OVERLAP) frames and between the passes of a progressive frame: the frames, the
    accumulators and the RNG states are bit-identical to the run without the queries, chain_report() and an armed frame
    event are the render launches' alone, and the query results are right.  default, trianglesOnly (the split launch,
    whose overlapped frames are really in flight), 64x40x4."""
    import torch

    tris, spheres, _, cam = tr.geometry("default")
    ds = rt.DeviceScene(tris, spheres)
    scene = rt.default_scene()
    W, H = tr.SHAPE
    cfg = rt.RenderConfig(W, H, 4, 10, True)
    ocfg = rt.RenderConfig(W, H, 4, 10, True, overlap=True)
    rays = tr.replay("default")
    e = tr.expected(tris, spheres, 1, rays)
    lim = oc.limits("median", e["prim"], e["depth"])
    want = oc.expected(tris, spheres, 1, rays, lim)
    d = _dev(rays)
    query = lambda flags=0: ds.occluded(d, lim, True, flags, count=True)  # noqa: E731
    right = lambda got: np.array_equal(got[0], want) and got[1] == int(want.sum())  # noqa: E731
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            first = _frame(ds, scene, cam, cfg, st)
            st.synchronize()
            report = ds.chain_report()
            assert right(query())
            assert ds.chain_report() == report
            # one pipelined triple on the frame event, queries between the frames on the same stream
            f1 = _frame(ds, scene, cam, ocfg, st, event=True)
            q1 = query()
            f2 = _frame(ds, scene, cam, ocfg, st, event=True)
            q2 = query(rt.RTC_F_NO_CLUSTER_CULL)
            f3 = _frame(ds, scene, cam, ocfg, st, event=True)
            for f in (f1, f2, f3):
                f[2].synchronize()
                assert _same(first, f)
            assert right(q1) and right(q2)
            torch.cuda.synchronize()
            report = ds.chain_report()
            # an armed frame event survives a query: the next render launch records it
            ev = torch.cuda.Event()
            ev.record(st)
            ds.set_frame_event(ev.cuda_event)
            assert right(query())
            assert ds.chain_report() == report
            col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            st.synchronize()
            ds.render_rows_async(scene, cam, ocfg, col.data_ptr(), None, None, st.cuda_stream)
            ev.synchronize()
            assert np.array_equal(col.cpu().numpy(), first[0].cpu().numpy()), "the frame event was not the render's"
            torch.cuda.synchronize()
            # one four-pass progressive frame: colours, accumulator and RNG states against the run without queries
            runs = []
            for with_queries in (False, True):
                col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
                acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
                rng = torch.zeros((H, W), dtype=torch.int32, device="cuda")
                st.synchronize()
                for k in range(4):
                    ds.render_samples_async(scene, cam, cfg, k, 1, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None,
                                            st.cuda_stream)
                    if with_queries:
                        assert right(query(FLAGS[k % 2]))
                st.synchronize()
                runs.append((col, acc, rng))
            assert _same(runs[0], runs[1]) and np.array_equal(runs[0][2].cpu().numpy(), runs[1][2].cpu().numpy())
            assert _same(first, runs[1])
    finally:
        torch.cuda.synchronize()
        ds.close()


def test_entry_points_and_inputs_agree(gpu_available):
    """rtc_occluded (host arrays: numpy RAY_DT and float32 [n, 6]; scalar, array and no limits) agrees with the
    asynchronous path (torch tensors), and all of them with the oracle."""
    import torch

    tris, spheres, tonly, _ = tr.geometry("default")
    rays, ds = tr.replay("default"), _scene("default")
    flat = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6)
    e = tr.case_expected("replay", "default")
    med = float(np.median(e["depth"][e["prim"] != -1]))
    for flags in FLAGS:
        for lim in (None, med, oc.case_limits("replay", "default", "above")):
            want = oc.expected(tris, spheres, tonly, rays, lim)
            host, hc = ds.occluded(rays, lim, False, flags, count=True)
            other = ds.occluded(flat, lim, False, flags)
            tl = torch.from_numpy(np.array(lim)).cuda() if isinstance(lim, np.ndarray) else lim
            dev, dc = ds.occluded(_dev(rays), tl, False, flags, count=True)
            assert np.array_equal(host, want) and np.array_equal(other, want) and np.array_equal(dev, want)
            assert hc == dc == int(want.sum())
            assert host.dtype == dev.dtype == bool and host.shape == dev.shape == (len(rays),)
    assert ds.occluded(rays[:100], 1.0, True).shape == (100,)


@pytest.mark.parametrize("limits", [False, True])
@pytest.mark.parametrize("outputs", ["bytes", "count"])
def test_host_entry_single_outputs(outputs, limits, gpu_available):
    """rtc_occluded itself (the Python method always asks for the bytes) with the bytes alone and with the count alone, with
    limits and with a null tMax, 65 rays -- a wave and one lane -- on the default scene: the device-tensor entry's answers
    for the same rays; the counter is added to, and left alone when not asked for."""
    import ctypes as C

    import torch

    ptr = rt._abi._ptr
    rays, ds = np.ascontiguousarray(tr.replay("default")[:65]), _scene("default")
    lim = np.ascontiguousarray(oc.case_limits("replay", "default", "above")[:65], F) if limits else None
    for flags in FLAGS:
        dev, dc = ds.occluded(_dev(rays), torch.from_numpy(lim.copy()).cuda() if limits else None, False, flags, count=True)
        occ, cnt = np.full(65, GUARD, np.uint8), C.c_ulonglong(1000)
        rc = rt.lib().rtc_occluded(ds._h, ptr(rays), ptr(lim), 65, 0, flags, ptr(occ) if outputs == "bytes" else None,
                                   C.cast(C.pointer(cnt), C.c_void_p) if outputs == "count" else None)
        assert rc == 0, flags
        assert np.array_equal(occ, dev.astype(np.uint8) if outputs == "bytes" else np.full(65, GUARD, np.uint8)), flags
        assert cnt.value == 1000 + (dc if outputs == "count" else 0), flags
        assert 0 < dc == int(dev.sum())


def test_refusals_on_a_scene(gpu_available):
    """On a real handle: an unknown flag and two null outputs are RTC_EINVAL with nothing enqueued; n == 0 writes nothing;
    no entry point takes 0x8000 (the deleted RTC_F_NO_REACH_CULL's bit)."""
    import torch

    ds, rays = _scene("suze"), _dev(tr.replay("suze"))
    n = len(rays)
    buf = torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    with pytest.raises(rt.RtcError) as ei:
        ds.occluded_async(rays.data_ptr(), n, 0, True, rt.RTC_F_NO_TILE_CULL, buf.data_ptr(), cnt.data_ptr())
    assert ei.value.code == rt._abi.RTC_EINVAL and "rtc_occluded_async" in str(ei.value)
    with pytest.raises(rt.RtcError):
        ds.occluded_async(rays.data_ptr(), n, 0, True, 0)
    ds.occluded_async(rays.data_ptr(), 0, 0, True, 0, buf.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all() and int(cnt.cpu().numpy()[0]) == 7
    with pytest.raises(rt.RtcError):
        ds.occluded_async(rays.data_ptr(), n, 0, True, 0x8000, buf.data_ptr(), cnt.data_ptr())
    with pytest.raises(rt.RtcError):
        ds.trace_rays_async(rays.data_ptr(), n, True, 0x8000, depth_ptr=0x1000)
    cfg = rt.RenderConfig(64, 40, 0, 0, True)
    cfg_flags = cfg.desc()
    cfg_flags.flags = 0x8000
    out = rt.RtcHitBuffers(buf.data_ptr(), None, None, None)
    import ctypes as C

    cam = tr.geometry("suze")[3]
    assert rt.lib().rtc_render_first_hit_async(ds._h, C.byref(cam), C.byref(cfg_flags), C.byref(out), None) == rt._abi.RTC_EINVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all()
    assert np.array_equal(ds.occluded(rays, None, True), oc.case_occluded("replay", "suze", "none"))
