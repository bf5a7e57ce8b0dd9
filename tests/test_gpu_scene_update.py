"""rtc_scene_update / rtc_scene_update_async on the GPU: a resident scene's triangles and spheres replaced in place by the
refit kernel (rtc_scene.hip rtc_refit), on every route of the renderer.  The records the kernel writes are compared byte
for byte with the host statement (rtc_scene_records_host, itself checked in tests/test_refit_host.py); the frames with
the CPU oracle's render of the NEW geometry: float bits, u8 and segment counts.  Every frame test first asserts with the
oracle, before it touches the GPU, that the move changes at least 5 % of the pixels and leaves geometry in view, so that
an update that did nothing, or half of it, cannot pass.  No reference counterpart: main.c:229-243 builds its arrays once;
the frames are raytracing.c's for the moved arrays."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import oracle.binding as orc
import raytracingc_amd as rt
from adversarial_scenes import SCENES as ADVERSARIAL
from conftest import load_tris, scene_spheres
from moving_scenes import HELPERS, shift, synthetic
from raytracingc_amd._abi import RtcRenderDesc, TRIANGLE_DT
from sphere_scenes import open5
from test_gpu_adversarial_frames import NAMES as ADVERSARIAL_NAMES

pytestmark = pytest.mark.gpu

COUNTS = (1, 7, 8, 9, 255, 256, 257, 264)
# per scene a camera close enough that the model fills a good part of a small frame (chosen on the CPU so that every
# helper used with the scene meets the 5 % condition below; the default camera sees the models in ~4 % of the pixels)
CAMERAS = {
    "ultracomplex": ((-4.24, -1.5, 4.24), (0.0, 0.0, 0.0), 2.5),
    "cube": ((-4.0, -3.08, 0.0), (0.0, -1.58, 0.0), 3.5),
    "fsuzane": ((0.0, -2.7, -6.0), (0.0, -1.2, 0.0), 2.5),
    "suzannes": (rt.DEFAULT_ORIGIN, (0.0, 0.0, 0.0), 2.5),
}
ROUTES = {
    "joined": dict(), "hoisted": dict(hoist=True), "no_coop": dict(coop=False), "no_tile_cull": dict(tile_cull=False),
    "no_cluster_cull": dict(cluster_cull=False), "debug": dict(debug_bounces=True), "pipelined": dict(overlap=True),
}
MIN_CHANGED = 0.05


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _tris(name):
    t = synthetic(int(name[1:])) if name[0] == "n" and name[1:].isdigit() else load_tris(name)[0]
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _moved(name, helper):
    t = _tris(name) if helper is None else HELPERS[helper](_tris(name))
    t.setflags(write=False)
    return t


def _camera(name):
    return rt.camera_basis(*CAMERAS[name])


def _oracle_render(tris, spheres, cam, W, H, spp, flags=0, max_bounce=10, rows=(0, 1)):
    d = RtcRenderDesc(W, H, spp, max_bounce, int(spheres is None or len(spheres) == 0), rows[0], rows[1], flags, 0)
    col, acc, seg = orc.render(tris, spheres, rt.default_scene(), cam, d, threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


@functools.lru_cache(maxsize=None)
def _oracle(name, helper, shape, debug=False):
    """The oracle's (u8, floats, segments) of scene `name` moved by `helper` (None: as loaded), computed once."""
    W, H, spp = shape
    return _oracle_render(_moved(name, helper), None, _camera(name), W, H, spp, rt.RTC_F_DEBUG_BOUNCES if debug else 0)


@functools.lru_cache(maxsize=None)
def _sky(name, shape):
    W, H, spp = shape
    return _oracle_render(_tris(name)[:0], None, _camera(name), W, H, spp)[0]


def _assert_move_shows(name, helper, shape):
    """With the oracle alone: the moved frame differs from the unmoved one in at least 5 % of the pixels and still has
    geometry pixels (pixels that differ from the empty scene's)."""
    a, b = _oracle(name, None, shape)[0], _oracle(name, helper, shape)[0]
    changed = float((a != b).any(-1).mean())
    assert changed >= MIN_CHANGED, f"{name} {helper}: only {changed:.3f} of the pixels change"
    assert (b != _sky(name, shape)).any(), f"{name} {helper}: no geometry pixel left"


def _launch(ds, cam, cfg, stream=None, counters=False, frame_event=False):
    """One launch into fresh buffers; returns (Color tensor, accumulator tensor, counter tensor or None)."""
    import torch

    rows = cfg.rows()
    out = torch.zeros((rows, cfg.width, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((rows, cfg.width, 3), dtype=torch.float32, device="cuda")
    seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
    torch.cuda.synchronize()  # (the fills ran on the current stream)
    if frame_event:
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream())
        ds.set_frame_event(ev.cuda_event)
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    ds.render_rows_async(rt.default_scene(), cam, cfg, out.data_ptr(), acc.data_ptr(), seg.data_ptr() if counters else None, st)
    return out, acc, seg


def _assert_frame(got, want, what, nan_ok=False):
    import torch

    torch.cuda.synchronize()
    out, acc, seg = got
    ocol, oacc, oseg = want
    a = acc.cpu().numpy()
    nan = np.isnan(oacc) if nan_ok else np.zeros(oacc.shape, bool)
    assert np.array_equal(np.isnan(a), np.isnan(oacc)), f"{what}: NaN positions differ"
    bad = int(((_bits(a) != _bits(oacc)) & ~nan).any(-1).sum())
    assert bad == 0, f"{what}: {bad} pixels' accumulator bits differ"
    col = out.cpu().numpy()
    assert np.array_equal(col, ocol), f"{what}: {int((col != ocol).any(-1).sum())} u8 pixels differ"
    if seg is not None:
        assert int(seg.cpu().numpy()[0]) == oseg, f"{what}: segments {int(seg.cpu().numpy()[0])} vs {oseg}"


def _assert_records(got, want, what, nan_ok=False):
    for name in rt.RECORD_ARRAYS:
        g, w = got[name], want[name]
        assert g.shape == w.shape, f"{what}: {name} {g.shape} vs {w.shape}"
        same = g == w
        if nan_ok:  # (gfx950 and x86 may give an invalid operation's NaN another sign; the NaN positions must agree)
            same |= np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32))
        assert same.all(), f"{what}: {int((~same).any(-1).sum())} records of {name} differ (first: {np.argwhere(~same)[:1]})"


# ---- 3. the records ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("helper", sorted(HELPERS))
@pytest.mark.parametrize("name", [f"n{n}" for n in COUNTS] + ["ultracomplex", "suzannes"])
def test_refit_records_equal_the_host_statement(name, helper, gpu_available):
    """Upload, update to helper(t): every record of the current generation equals rtc_scene_records_host(t, helper(t)) byte
    for byte; then a second update back to t (the other generation): the upload's own records."""
    t, moved = _tris(name), _moved(name, helper)
    ds = rt.DeviceScene(t, None)
    try:
        _assert_records(ds.records(), rt.scene_records_host(t), f"{name} upload")
        ds.update(moved)
        _assert_records(ds.records(), rt.scene_records_host(t, moved), f"{name} {helper}")
        ds.update(t)
        _assert_records(ds.records(), rt.scene_records_host(t), f"{name} {helper} and back")
    finally:
        ds.close()


# ---- 4. frames on every route -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("helper", ["shift", "squash"])
@pytest.mark.parametrize("name", ["ultracomplex", "cube", "fsuzane"])
def test_frames_before_and_after_an_update(name, helper, route, gpu_available):
    """Geometry A, an update to B with the same camera, geometry B: both frames are the oracle's.  The pipelined route
    updates through a device tensor on a stream of its own (rtc_scene_update_async), the others through numpy."""
    import torch

    shape = (96, 54, 8)
    _assert_move_shows(name, helper, shape)
    debug = route == "debug"
    want_a, want_b = _oracle(name, None, shape, debug), _oracle(name, helper, shape, debug)
    cam, cfg = _camera(name), rt.RenderConfig(*shape, 10, True, **ROUTES[route])
    pipelined = route == "pipelined"
    st = torch.cuda.Stream() if pipelined else None
    counters = not pipelined  # (a launch that counts segments is a joined one)
    ds = rt.DeviceScene(_tris(name), None)
    try:
        a = _launch(ds, cam, cfg, st, counters, frame_event=pipelined)
        if pipelined:
            dev = torch.from_numpy(_moved(name, helper).copy().view(np.uint8)).cuda()
            torch.cuda.synchronize()
            ds.update(tris=dev, stream=st.cuda_stream)
        else:
            ds.update(_moved(name, helper))
        b = _launch(ds, cam, cfg, st, counters, frame_event=pipelined)
        _assert_frame(a, want_a, f"{name} {route} before the update")
        _assert_frame(b, want_b, f"{name} {helper} {route} after the update")
    finally:
        ds.close()


# ---- 5. scatter: the clusters lose their locality ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ultracomplex", "suzannes"])
def test_scattered_triangles_render_exactly(name, gpu_available):
    """After `scatter` the balls are huge and the chunk balls overlap: the culling only loosens.  The frame and the segment
    count are the oracle's, with the cluster cull and (the same handle) without it."""
    shape = (64, 40, 8)
    _assert_move_shows(name, "scatter", shape)
    want = _oracle(name, "scatter", shape)
    cam = _camera(name)
    ds = rt.DeviceScene(_tris(name), None)
    try:
        ds.update(_moved(name, "scatter"))
        for kw in (dict(), dict(cluster_cull=False)):
            got = _launch(ds, cam, rt.RenderConfig(*shape, 10, True, **kw), counters=True)
            _assert_frame(got, want, f"{name} scatter {kw}")
    finally:
        ds.close()


# ---- 6. spheres -------------------------------------------------------------------------------------------------------
def test_default_scene_sphere_moves_alone(gpu_available):
    """The reference's default box: its sphere moved and resized, the triangles left alone (a null triangle pointer), on the
    one-lane-per-pixel route the closed box takes."""
    t = load_tris("default")[0]
    s0 = scene_spheres("default")
    s1 = s0.copy()
    s1["pos"]["x"], s1["pos"]["y"], s1["r"] = 1.5, 0.25, 1.25
    cam, shape = rt.camera_basis(), (96, 54, 4)
    want0, want1 = (_oracle_render(t, s, cam, *shape) for s in (s0, s1))
    assert (want0[0] != want1[0]).any(-1).mean() >= MIN_CHANGED
    cfg = rt.RenderConfig(*shape, 10, False)
    ds = rt.DeviceScene(t, s0)
    try:
        assert not ds.sphere_split
        a = _launch(ds, cam, cfg, counters=True)
        ds.update(spheres=s1)
        b = _launch(ds, cam, cfg, counters=True)
        _assert_frame(a, want0, "default before")
        _assert_frame(b, want1, "default sphere moved")
        rec, host = ds.records(), rt.scene_records_host(t, None, s1)
        _assert_records(rec, host, "default sphere moved")
    finally:
        ds.close()


@pytest.mark.parametrize("split", [True, False])
def test_open_sphere_scene_moves(split, gpu_available):
    """An open sphere scene (the sphere split's gate allows it): one sphere and every third triangle moved in one update,
    through the split launch and, with RTC_F_NO_COOP, one lane per pixel."""
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
        a = _launch(ds, cam, cfg, counters=True)
        ds.update(t1, s1)
        b = _launch(ds, cam, cfg, counters=True)
        _assert_frame(a, want0, f"open5 split={split} before")
        _assert_frame(b, want1, f"open5 split={split} after")
        _assert_records(ds.records(), rt.scene_records_host(t, t1, s1), "open5 moved")
    finally:
        ds.close()


# ---- 7. adversarial targets -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ADVERSARIAL_NAMES)
def test_update_to_adversarial_geometry(name, gpu_available):
    """A benign scene of the same size (one unit triangle repeated) updated to each adversarial scene: the frame is the
    oracle's (NaN positions equal, every other float bit-equal), the records the host statement's."""
    tris, cam, _ = ADVERSARIAL[name]
    benign = np.zeros(len(tris), TRIANGLE_DT)
    benign["posB"]["x"] = benign["posC"]["y"] = 1.0
    benign["posA"]["z"] = benign["posB"]["z"] = benign["posC"]["z"] = 3.0
    benign["normal"]["z"] = -1.0
    W, H, spp, mb = 48, 40, 6, 4
    want = _oracle_render(tris, None, cam, W, H, spp, 0, mb)
    ds = rt.DeviceScene(benign, None)
    try:
        ds.update(tris)
        got = _launch(ds, cam, rt.RenderConfig(W, H, spp, mb, True), counters=True)
        _assert_frame(got, want, name, nan_ok=True)
        _assert_records(ds.records(), rt.scene_records_host(benign, tris), name, nan_ok=True)
    finally:
        ds.close()


# ---- 8. pipelined animation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [False, True])
def test_pipelined_animation(share, gpu_available):
    """12 overlapped launches, an update (device tensors, the launch stream) before each: whole frames of 1000 x 700 x 4 (the
    alternating cull streams) or a 1/8 row share of 1920 x 1080 x 4 (the merged sky pass), into three Color buffers, each
    consumed late on another stream.  Frame k's triangles are `shift` scaled by k / 12: every frame equals the oracle's
    frame of its own geometry -- a frame rendered with its successor's records, or an update that overwrote records still
    being read, differs."""
    import torch

    n = 12
    t, cam = _tris("ultracomplex"), _camera("ultracomplex")
    W, H, spp = (1920, 1080, 4) if share else (1000, 700, 4)
    rows = (3, 8) if share else (0, 1)
    geoms = [shift(t, k / n) for k in range(n)]
    want = [_oracle_render(g, None, cam, W, H, spp, rows=rows)[0] for g in geoms]
    assert all((want[k] != want[k + 1]).any() for k in range(n - 1)), "successive frames must differ"
    cfg = rt.RenderConfig(W, H, spp, 10, True, overlap=True, row_start=rows[0], row_stride=rows[1])
    dev = [torch.from_numpy(g.view(np.uint8)).cuda() for g in geoms]
    ds = rt.DeviceScene(t, None)
    st, cp = torch.cuda.Stream(), torch.cuda.Stream()
    nb = 3
    bufs = [torch.zeros((cfg.rows(), W, 3), dtype=torch.uint8, device="cuda") for _ in range(nb)]
    torch.cuda.synchronize()
    freed, got = [None] * nb, []
    try:
        for k in range(n):
            b = k % nb
            if freed[b] is not None:  # buffer b is rewritten only after its previous frame was copied
                st.wait_event(freed[b])
            ds.update(tris=dev[k], stream=st.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(st)  # (a torch event has no hipEvent_t until its first record)
            ds.set_frame_event(ev.cuda_event)
            ds.render_rows_async(rt.default_scene(), cam, cfg, bufs[b].data_ptr(), stream=st.cuda_stream)
            cp.wait_event(ev)
            with torch.cuda.stream(cp):
                if hasattr(torch.cuda, "_sleep"):
                    torch.cuda._sleep(2_000_000)  # ~1 ms: the copy runs late, the next updates and frames are queued by then
                got.append(bufs[b].clone())
                freed[b] = torch.cuda.Event()
                freed[b].record(cp)
        torch.cuda.synchronize()
        for k, g in enumerate(got):
            bad = int((g.cpu().numpy() != want[k]).any(-1).sum())
            assert bad == 0, f"frame {k}: {bad} pixels differ from the oracle's frame of its own geometry"
    finally:
        torch.cuda.synchronize()
        ds.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------
def test_refused_updates_change_nothing(gpu_available):
    """Wrong counts, both pointers null and a null scene return RTC_EINVAL with nothing enqueued: the next frame is the old
    geometry's, bit for bit.  An update on a released handle raises."""
    import torch

    name, shape = "ultracomplex", (96, 54, 8)
    t, moved = _tris(name), _moved(name, "shift")
    L, cam, cfg = rt.lib(), _camera(name), rt.RenderConfig(*shape, 10, True)
    dev = torch.from_numpy(moved.copy().view(np.uint8)).cuda()
    torch.cuda.synchronize()
    p = C.c_void_p(dev.data_ptr())
    ds = rt.DeviceScene(t, None)
    try:
        h = ds._h
        assert L.rtc_scene_update_async(None, p, len(t), None, 0, None) == rt.RTC_EINVAL
        assert L.rtc_scene_update_async(h, None, 0, None, 0, None) == rt.RTC_EINVAL
        assert L.rtc_scene_update_async(h, p, len(t) - 1, None, 0, None) == rt.RTC_EINVAL
        assert L.rtc_scene_update_async(h, p, len(t), p, 1, None) == rt.RTC_EINVAL  # (a scene without spheres)
        assert L.rtc_scene_update_async(h, None, len(t), None, 0, None) == rt.RTC_EINVAL
        assert L.rtc_scene_update(None, None, 0, None, 0) == rt.RTC_EINVAL
        with pytest.raises(rt.RtcError):
            ds.update(moved[:-1])
        with pytest.raises(ValueError):
            ds.update()
        _assert_frame(_launch(ds, cam, cfg, counters=True), _oracle(name, None, shape), "after the refused updates")
        _assert_records(ds.records(), rt.scene_records_host(t), "after the refused updates")
    finally:
        ds.close()
    with pytest.raises(RuntimeError):
        ds.update(moved)
    with pytest.raises(RuntimeError):
        ds.records()
