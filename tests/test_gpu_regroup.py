"""rtc_scene_regroup / rtc_scene_regroup_async on the GPU: a resident scene's clusters decided anew on the
device from moved triangles, then the refit.  The acceptance is exactness: after DeviceScene(t0) and update(t1,
regroup=True) the six record arrays equal rtc_scene_records_host(t1) -- a fresh upload of t1 -- byte for byte, and a later
update(t2) refits that grouping; the frames before and after are the oracle's on every route, in two passes, with spheres
and on the adversarial tie scenes (the membership must not leak into tie-breaks); the three ray queries answer as without
the cluster cull and as on a fresh upload; pipelined frames around regroups are each their own geometry's; refused calls
change nothing.  And it helps: on a scattered scene the segments stay and the tests fall.  Helpers, scenes, cameras and
oracle frames are tests/test_gpu_scene_update.py's (computed once, shared).  No reference counterpart: main.c:229-243
builds its arrays once."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import raytracingc_amd as rt
from adversarial_scenes import SCENES as ADVERSARIAL
from conftest import load_tris, scene_spheres
from moving_scenes import HELPERS, VERTS, scatter, shift, synthetic
from primary_rays import launch_rays
from raytracingc_amd._abi import TRIANGLE_DT
from sphere_scenes import open5
from test_gpu_adversarial_frames import NAMES as ADVERSARIAL_NAMES
from test_gpu_scene_update import (MIN_CHANGED, ROUTES, _assert_frame, _assert_move_shows, _assert_records, _camera, _launch,
                                   _moved, _oracle, _oracle_render, _tris)
from test_regroup_host import _poisoned, at

pytestmark = pytest.mark.gpu

NAMES = [f"n{n}" for n in (1, 7, 8, 9, 17, 25, 255, 256, 257, 264, 513, 2049)] + ["ultracomplex", "suzannes"]
WAVE, NO_CULL = rt.RTC_F_WAVE_PER_RAY, rt.RTC_F_NO_CLUSTER_CULL


def _device(t):
    import torch

    dev = torch.from_numpy(np.ascontiguousarray(t, TRIANGLE_DT).copy().view(np.uint8)).cuda()
    torch.cuda.synchronize()
    return dev


# ---- 1. the records -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("helper", sorted(HELPERS))
@pytest.mark.parametrize("name", NAMES)
def test_records_equal_a_fresh_upload(name, helper, gpu_available):
    """DeviceScene(t0), update(t1, regroup=True): the records are rtc_scene_records_host(t1)'s, a fresh upload's; a following
    update(t0) refits that grouping: rtc_scene_records_host(t1, t0).  `scatter` goes through a device tensor
    (rtc_scene_regroup_async on torch's current stream), the others through numpy (rtc_scene_regroup)."""
    import torch

    t0, t1 = _tris(name), _moved(name, helper)
    ds = rt.DeviceScene(t0, None)
    try:
        if helper == "scatter":
            ds.update(tris=_device(t1), regroup=True)
            torch.cuda.synchronize()
        else:
            ds.update(t1, regroup=True)
        _assert_records(ds.records(), rt.scene_records_host(t1), f"{name} {helper} regrouped")
        ds.update(t0)
        _assert_records(ds.records(), rt.scene_records_host(t1, t0), f"{name} {helper} regrouped, then updated")
    finally:
        ds.close()


def _designed():
    n = 264
    i = np.arange(32)
    mixed = synthetic(n)
    for k, v in enumerate([np.nan, np.inf, -np.inf, 0.0, -0.0]):
        for vert in VERTS:
            mixed[vert]["x"][k::11] = v
    return {
        "equal_centroids": at(np.tile([[0.5, -1.0, 3.0]], (40, 1))),
        "ties_by_position": at(np.stack([-1.0 * i, 6.0 * (i // 2 % 4), np.zeros(32)], 1)),
        "equal_extents": at(np.stack([np.arange(16), (np.arange(16) * 5) % 16, (np.arange(16) * 7) % 16 / 32], 1)),
        "nan_some": _poisoned(n, slice(1, None, 5), np.nan), "nan_all": _poisoned(n, slice(None), np.nan, ("x", "y", "z")),
        "inf_some": _poisoned(n, slice(1, None, 5), np.inf), "inf_all": _poisoned(n, slice(None), np.inf),
        "neg_inf_posB": _poisoned(n, slice(1, None, 5), -np.inf, ("y",), ("posB",)),
        "neg_zero_all": _poisoned(n, slice(None), -0.0), "mixed": mixed,
    }


DESIGNED = _designed()


@pytest.mark.parametrize("name", sorted(DESIGNED) + ADVERSARIAL_NAMES)
def test_designed_inputs_regroup_as_an_upload_groups_them(name, gpu_available):
    """The inputs of tests/test_regroup_host.py that a rank count can get wrong, and every adversarial scene, as regroup
    targets of a benign scene of the same size (NaN positions equal, every other byte equal)."""
    t1 = DESIGNED[name] if name in DESIGNED else ADVERSARIAL[name][0]
    t0 = synthetic(len(t1))
    ds = rt.DeviceScene(t0, None)
    try:
        ds.update(t1, regroup=True)
        _assert_records(ds.records(), rt.scene_records_host(t1), name, nan_ok=True)
        ds.update(t0)
        _assert_records(ds.records(), rt.scene_records_host(t1, t0), f"{name}, then updated", nan_ok=True)
    finally:
        ds.close()


# ---- 2. frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name, helper", [("ultracomplex", "shift"), ("ultracomplex", "squash"), ("cube", "shift"),
                                          ("fsuzane", "squash")])
def test_frames_before_and_after_a_regroup(name, helper, route, gpu_available):
    """Geometry t0, a regroup to t1 with the same camera, geometry t1: both frames are the oracle's, and the second is a
    fresh DeviceScene(t1)'s.  The pipelined route regroups through a device tensor on the launch stream, which is not
    torch's current one."""
    import torch

    shape = (96, 54, 8)
    _assert_move_shows(name, helper, shape)
    debug = route == "debug"
    want_a, want_b = _oracle(name, None, shape, debug), _oracle(name, helper, shape, debug)
    cam, cfg = _camera(name), rt.RenderConfig(*shape, 10, True, **ROUTES[route])
    pipelined = route == "pipelined"
    st = torch.cuda.Stream() if pipelined else None
    counters = not pipelined
    ds, fresh = rt.DeviceScene(_tris(name), None), rt.DeviceScene(_moved(name, helper), None)
    try:
        a = _launch(ds, cam, cfg, st, counters, frame_event=pipelined)
        if pipelined:
            dev = _device(_moved(name, helper))
            ds.update(tris=dev, stream=st.cuda_stream, regroup=True)  # (the scratch: torch's current stream's, kept for st)
        else:
            ds.update(_moved(name, helper), regroup=True)
        b = _launch(ds, cam, cfg, st, counters, frame_event=pipelined)
        f = _launch(fresh, cam, cfg, st, counters, frame_event=pipelined)
        _assert_frame(a, want_a, f"{name} {route} before the regroup")
        _assert_frame(b, want_b, f"{name} {helper} {route} after the regroup")
        _assert_frame(f, want_b, f"{name} {helper} {route} fresh upload")
        assert torch.equal(b[1], f[1]) and torch.equal(b[0], f[0])
        if counters:
            assert torch.equal(b[2], f[2]), "every counter is a fresh upload's: the same records, the same work"
    finally:
        ds.close()
        fresh.close()


def test_two_passes_after_a_regroup(gpu_available):
    """A progressive frame (3 + 5 samples) of the regrouped scene: the finished frame is the oracle's."""
    name, helper, shape = "ultracomplex", "shift", (96, 54, 8)
    want = _oracle(name, helper, shape)
    cam, cfg = _camera(name), rt.RenderConfig(*shape, 10, True)
    ds = rt.DeviceScene(_tris(name), None)
    try:
        first = [acc for _, _, acc in ds.render_progressive(rt.default_scene(), cam, cfg, [3, 5])][-1]
        assert np.array_equal(first.view(np.uint32), _oracle(name, None, shape)[1].view(np.uint32).reshape(first.shape))
        ds.update(_moved(name, helper), regroup=True)
        got = list(ds.render_progressive(rt.default_scene(), cam, cfg, [3, 5]))
        assert [g[0] for g in got] == [3, 8]
        assert np.array_equal(got[-1][2].view(np.uint32), want[1].view(np.uint32).reshape(got[-1][2].shape))
        assert np.array_equal(got[-1][1], want[0].reshape(got[-1][1].shape))
    finally:
        ds.close()


def test_default_scene_regroups_with_its_sphere(gpu_available):
    """The reference's default box and sphere: a regroup of the shifted triangles that keeps the sphere (a null sphere
    pointer), then one that moves it too."""
    t = load_tris("default")[0]
    t1 = shift(t)
    s0 = scene_spheres("default")
    s1 = s0.copy()
    s1["pos"]["x"], s1["pos"]["y"], s1["r"] = 1.5, 0.25, 1.25
    cam, shape = rt.camera_basis(), (96, 54, 4)
    want = [_oracle_render(tt, ss, cam, *shape) for tt, ss in ((t, s0), (t1, s0), (t1, s1))]
    assert (want[0][0] != want[1][0]).any(-1).mean() >= MIN_CHANGED
    cfg = rt.RenderConfig(*shape, 10, False)
    ds = rt.DeviceScene(t, s0)
    try:
        a = _launch(ds, cam, cfg, counters=True)
        ds.update(t1, regroup=True)
        b = _launch(ds, cam, cfg, counters=True)
        _assert_records(ds.records(), rt.scene_records_host(t1, None, s0), "default regrouped, sphere kept")
        ds.update(t1, s1, regroup=True)
        c = _launch(ds, cam, cfg, counters=True)
        _assert_records(ds.records(), rt.scene_records_host(t1, None, s1), "default regrouped, sphere moved")
        for got, w, what in zip((a, b, c), want, ("before", "regrouped", "regrouped with the sphere")):
            _assert_frame(got, w, f"default {what}")
    finally:
        ds.close()


@pytest.mark.parametrize("split", [True, False])
def test_open_sphere_scene_regroups(split, gpu_available):
    """open5 around ultracomplex: one sphere and every third triangle moved in one regroup, through the split launch and,
    with RTC_F_NO_COOP, one lane per pixel; the gate keeps the upload's verdict."""
    t = _tris("ultracomplex")
    s0 = open5()
    s1 = s0.copy()
    s1[0]["pos"]["x"], s1[0]["pos"]["y"], s1[0]["r"] = 0.2, -2.2, 1.3
    t1 = shift(t)
    cam, shape = _camera("ultracomplex"), (96, 54, 4)
    want0, want1 = _oracle_render(t, s0, cam, *shape), _oracle_render(t1, s1, cam, *shape)
    assert (want0[0] != want1[0]).any(-1).mean() >= MIN_CHANGED
    cfg = rt.RenderConfig(*shape, 10, False, split_spheres=split, coop=split)
    ds = rt.DeviceScene(t, s0)
    try:
        gate, wgs, bounds = ds.sphere_split, ds.chain_wgs, ds.bounds()
        a = _launch(ds, cam, cfg, counters=True)
        ds.update(t1, s1, regroup=True)
        b = _launch(ds, cam, cfg, counters=True)
        _assert_frame(a, want0, f"open5 split={split} before")
        _assert_frame(b, want1, f"open5 split={split} after")
        _assert_records(ds.records(), rt.scene_records_host(t1, None, s1), "open5 regrouped")
        assert (ds.sphere_split, ds.chain_wgs) == (gate, wgs), "the upload's hints keep their values"
        assert all(np.array_equal(x, y) for x, y in zip(ds.bounds(), bounds))
    finally:
        ds.close()


@pytest.mark.parametrize("name", [n for n in ADVERSARIAL_NAMES if n.startswith("ties_")])
def test_regroup_to_tie_scenes(name, gpu_available):
    """The coplanar ties: which of two equal hits wins is decided by the reference index, whatever cluster order the
    regroup leaves (here from a benign scene whose upload grouped the indices otherwise)."""
    tris, cam, _ = ADVERSARIAL[name]
    benign = synthetic(len(tris))
    W, H, spp, mb = 48, 40, 6, 4
    want = _oracle_render(tris, None, cam, W, H, spp, 0, mb)
    ds = rt.DeviceScene(benign, None)
    try:
        ds.update(tris, regroup=True)
        for kw in (dict(), dict(cluster_cull=False)):
            got = _launch(ds, cam, rt.RenderConfig(W, H, spp, mb, True, **kw), counters=True)
            _assert_frame(got, want, f"{name} {kw}", nan_ok=True)
    finally:
        ds.close()


# ---- 3. queries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ultracomplex", "suzannes"])
def test_queries_on_a_regrouped_scene(name, gpu_available):
    """trace_rays, trace_paths (a lane and a wave per ray) and occluded (bytes and count) on a frame's rays: the regrouped
    scene answers word for word as it does without the cluster cull and as a fresh upload of the same triangles does."""
    t0, t1 = _tris(name), _moved(name, "scatter")
    cam = _camera(name)
    rays = launch_rays(cam, rt.RenderConfig(96, 54, 1, 10, True))
    seeds = (np.arange(len(rays), dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(12345)
    scene = rt.default_scene()
    ds, fresh = rt.DeviceScene(t0, None), rt.DeviceScene(t1, None)
    try:
        ds.update(t1, regroup=True)

        def answers(s, flags):
            out = dict(s.trace_rays(rays, True, flags=flags))
            for wave in (0, WAVE):
                p = s.trace_paths(rays, seeds, scene, 4, 4, True, flags=flags | wave, segments=True)
                out.update({f"radiance{wave}": p["radiance"].view(np.uint32), f"seeds{wave}": p["seeds"],
                            f"segments{wave}": np.array(p["segments"])})
            out["occluded"], count = s.occluded(rays, 8.0, True, flags=flags, count=True)
            out["count"] = np.array(count)
            return out

        base = answers(ds, 0)
        assert base["count"] > 0 and (base["prim"] >= 0).any(), "the rays must meet the geometry"
        for what, other in (("without the cluster cull", answers(ds, NO_CULL)), ("a fresh upload", answers(fresh, 0))):
            for k, v in base.items():
                w = other[k]
                same = (v == w) | (np.isnan(v) & np.isnan(w)) if v.dtype.kind == "f" else v == w
                assert same.all(), f"{name} {k} differs from {what}"
    finally:
        ds.close()
        fresh.close()


# ---- 4. pipelined -------------------------------------------------------------------------------------------------------
def test_pipelined_frames_around_regroups(gpu_available):
    """8 overlapped whole frames of 1000 x 700 x 4 on one stream (the alternating cull streams), an update (odd frames) or
    a regroup (even frames) from device tensors before each, into three Color buffers consumed late on another stream:
    every frame is the oracle's frame of its own geometry -- a regroup that rewrote records, or a membership, still being
    read would show."""
    import torch

    n = 8
    t, cam = _tris("ultracomplex"), _camera("ultracomplex")
    W, H, spp = 1000, 700, 4
    geoms = [shift(t, k / n) for k in range(n)]
    want = [_oracle_render(g, None, cam, W, H, spp)[0] for g in geoms]
    assert all((want[k] != want[k + 1]).any() for k in range(n - 1)), "successive frames must differ"
    cfg = rt.RenderConfig(W, H, spp, 10, True, overlap=True)
    dev = [_device(g) for g in geoms]
    ds = rt.DeviceScene(t, None)
    st, cp = torch.cuda.Stream(), torch.cuda.Stream()
    nb = 3
    bufs = [torch.zeros((cfg.rows(), W, 3), dtype=torch.uint8, device="cuda") for _ in range(nb)]
    scratch = torch.zeros(ds.regroup_scratch_bytes(), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    freed, got = [None] * nb, []
    try:
        for k in range(n):
            b = k % nb
            if freed[b] is not None:
                st.wait_event(freed[b])
            if k % 2:
                ds.update(tris=dev[k], stream=st.cuda_stream)
            else:
                ds.regroup_async(dev[k].data_ptr(), None, scratch.data_ptr(), scratch.numel(), st.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(st)
            ds.set_frame_event(ev.cuda_event)
            ds.render_rows_async(rt.default_scene(), cam, cfg, bufs[b].data_ptr(), stream=st.cuda_stream)
            cp.wait_event(ev)
            with torch.cuda.stream(cp):
                if hasattr(torch.cuda, "_sleep"):
                    torch.cuda._sleep(2_000_000)
                got.append(bufs[b].clone())
                freed[b] = torch.cuda.Event()
                freed[b].record(cp)
        torch.cuda.synchronize()
        for k, g in enumerate(got):
            bad = int((g.cpu().numpy() != want[k]).any(-1).sum())
            assert bad == 0, f"frame {k}: {bad} pixels differ from the oracle's frame of its own geometry"
        _assert_records(ds.records(), rt.scene_records_host(geoms[n - 2], geoms[n - 1]), "the last regroup, then the last update")
    finally:
        torch.cuda.synchronize()
        ds.close()


# ---- 5. it helps --------------------------------------------------------------------------------------------------------
def test_regroup_restores_the_culling(gpu_available, capsys):
    """scatter(suzannes): the same frame and the same segments after a stale update and after a regroup, and strictly fewer
    ray-triangle plus ray-ball tests after the regroup (the values are printed; DESIGN 3.16 records them; no ratio is
    fixed here)."""
    name, shape = "suzannes", (96, 54, 8)
    t0, t1 = _tris(name), _moved(name, "scatter")
    cam, cfg = _camera(name), rt.RenderConfig(*shape, 10, True)
    seg = {}
    frames = {}
    for regroup in (False, True):
        ds = rt.DeviceScene(t0, None)
        try:
            ds.update(t1, regroup=regroup)
            out, acc, s = _launch(ds, cam, cfg, counters=True)
            seg[regroup] = s.cpu().numpy().astype(np.int64)
            frames[regroup] = acc.cpu().numpy().view(np.uint32)
        finally:
            ds.close()
    with capsys.disabled():
        print(f"\nscatter(suzannes) {shape}: stale counters {seg[False].tolist()}, regrouped {seg[True].tolist()}")
    assert np.array_equal(frames[False], frames[True])
    assert seg[False][0] == seg[True][0] > 0
    assert seg[True][2] + seg[True][3] < seg[False][2] + seg[False][3]


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refused_regroups_change_nothing(gpu_available):
    """Bad counts, a null dTris, a null, small or misaligned scratch, a kind the scene lacks: RTC_EINVAL, nothing enqueued;
    the records and the next frame are the old geometry's."""
    name, shape = "ultracomplex", (96, 54, 8)
    t, moved = _tris(name), _moved(name, "shift")
    L, cam, cfg = rt.lib(), _camera(name), rt.RenderConfig(*shape, 10, True)
    import torch

    dev = _device(moved)
    p, n = C.c_void_p(dev.data_ptr()), len(t)
    ds = rt.DeviceScene(t, None)
    try:
        h, need = ds._h, ds.regroup_scratch_bytes()
        assert need > 0 and need % 16 == 0 and need >= 32 * n
        scratch = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sp = scratch.data_ptr()
        assert sp % 16 == 0
        q = C.c_void_p(sp)
        E = rt.RTC_EINVAL
        assert L.rtc_scene_regroup_async(None, p, n, None, 0, q, need, None) == E
        assert L.rtc_scene_regroup_async(h, None, 0, None, 0, q, need, None) == E
        assert L.rtc_scene_regroup_async(h, None, n, None, 0, q, need, None) == E
        assert L.rtc_scene_regroup_async(h, p, n - 1, None, 0, q, need, None) == E
        assert L.rtc_scene_regroup_async(h, p, n + 1, None, 0, q, need + 64, None) == E
        assert L.rtc_scene_regroup_async(h, p, n, p, 1, q, need, None) == E  # (a scene without spheres)
        assert L.rtc_scene_regroup_async(h, p, n, None, 0, None, need, None) == E
        assert b"scratch" in L.rtc_last_error()
        assert L.rtc_scene_regroup_async(h, p, n, None, 0, q, need - 1, None) == E
        assert L.rtc_scene_regroup_async(h, p, n, None, 0, q, 0, None) == E
        assert L.rtc_scene_regroup_async(h, p, n, None, 0, C.c_void_p(sp + 8), need, None) == E
        assert L.rtc_scene_regroup(h, None, 0, None, 0) == E
        assert L.rtc_scene_regroup(h, moved.ctypes.data_as(C.c_void_p), n - 1, None, 0) == E
        with pytest.raises(rt.RtcError):
            ds.update(moved[:-1], regroup=True)
        with pytest.raises(ValueError):
            ds.update(spheres=scene_spheres("default"), regroup=True)
        _assert_frame(_launch(ds, cam, cfg, counters=True), _oracle(name, None, shape), "after the refused regroups")
        _assert_records(ds.records(), rt.scene_records_host(t), "after the refused regroups")
        # and the same arguments, whole, are taken
        assert L.rtc_scene_regroup_async(h, p, n, None, 0, q, need, None) == 0
        _assert_records(ds.records(), rt.scene_records_host(moved), "after the regroup that was taken")
    finally:
        ds.close()
    with pytest.raises(RuntimeError):
        ds.update(moved, regroup=True)


def test_more_triangles_than_the_cap_are_refused(gpu_available):
    """A scene of one triangle more than rtc_scene_regroup_max_tris(): the message says to upload again; an update still
    works."""
    n = rt.regroup_max_tris() + 1
    rng = np.random.default_rng(11)
    t = at(rng.uniform(-3.0, 3.0, (n, 3)) + [0.0, 0.0, 6.0])
    ds = rt.DeviceScene(t, None)
    try:
        with pytest.raises(rt.RtcError, match="upload again"):
            ds.update(t, regroup=True)
        ds.update(t)
    finally:
        ds.close()
