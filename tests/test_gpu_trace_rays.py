"""rtc_trace_rays_async / rtc_trace_rays on the GPU (include/rtc.h): the four buffers -- primitive id, depth,
normal, albedo -- of caller-supplied rays against the CPU oracle's calculateRayCollision (raytracing.c:216-240;
tests/trace_rays_reference.py), compared as uint32 bit patterns for every ray, no tolerance.  One exception: where an
expected normal word of a sphere hit is NaN the result must be NaN, sign and payload free (tr.differing).  Every set runs
with the cluster cull and with RTC_F_NO_CLUSTER_CULL.  The sets' premises (hits and misses occur, rays beyond the cull's
bound hit, scales change winners, the one NaN) are tests/test_trace_rays_reference.py's, without a GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import moving_scenes
import raytracingc_amd as rt
import trace_rays_reference as tr

pytestmark = pytest.mark.gpu

ZERO = dict.fromkeys(tr.NAMES, 0)
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
FLAGS = [0, NO_CULL]
WORDS = {"prim": 1, "depth": 1, "normal": 3, "albedo": 3}
GUARD = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def _scene(name):
    tris, spheres = tr.geometry(name)[:2]
    return rt.DeviceScene(tris, spheres)


def _dev(rays):
    """The rays as a float32 [n, 6] tensor on the device."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6).copy()).cuda()


def _trace(ds, rays, tonly, flags, want=tr.NAMES):
    return ds.trace_rays(_dev(rays), bool(tonly), want, flags)


def _check(ds, rays, tonly, want_all, what):
    """Both paths against the expectation; returns the cull path's buffers."""
    got = None
    for flags in FLAGS:
        g = _trace(ds, rays, tonly, flags)
        bad = tr.differing(g, want_all)
        print(f"{what} flags {flags:#x}: {len(rays)} rays, differing {bad}")
        assert set(g) == set(tr.NAMES) and bad == ZERO, f"{what} flags {flags:#x}"
        got = got or g
    return got


@pytest.mark.parametrize("kind", ["primary", "replay"])
@pytest.mark.parametrize("name", sorted(tr.REPLAY))
def test_named_sets(name, kind, gpu_available):
    """The primary rays and the recorded bounce rays of every case, all four buffers, both paths."""
    tonly = tr.geometry(name)[2]
    got = _check(_scene(name), tr.case_rays(kind, name), tonly, tr.case_expected(kind, name), f"{kind} {name}")
    if kind == "replay":
        assert int((got["prim"] != -1).sum()) == tr.REPLAY[name][1]


@pytest.mark.parametrize("scale", tr.SCALES)
@pytest.mark.parametrize("name", tr.SCALED_CASES)
def test_scaled_sets(name, scale, gpu_available):
    """dir times 0.25, 3 (|dir|_1 beyond the cull's bound: those lanes must keep every ball), 1e-3 and 1e4 (the EPSILON
    tests see the caller's scale: the direction is not normalised)."""
    _check(_scene(name), tr.scaled(name, scale), 1, tr.case_expected("scaled", name, scale), f"scaled {name} x{scale}")


@pytest.mark.parametrize("tonly", [0, 1])
def test_odd_rays(tonly, gpu_available):
    """NaN, infinite, zero, tiny and huge components against the default scene, with and without its sphere."""
    got = _check(_scene("default"), tr.odd()[0], tonly, tr.case_expected("odd", "default", None, tonly), f"odd tonly {tonly}")
    if not tonly:
        assert np.isnan(got["normal"][tr.odd()[1].index("dir = 0 from the centre")]).all()


def test_spheres_present_but_skipped(gpu_available):
    """trianglesOnly = 1 on the default scene's replay rays: the sphere is resident and must not be seen."""
    tris, spheres, _, _ = tr.geometry("default")
    rays = tr.replay("default")
    want = tr.expected(tris, spheres, 1, rays)
    with_sphere = tr.case_expected("replay", "default")
    assert (want["prim"] >= -1).all() and (want["prim"] != with_sphere["prim"]).sum() >= tr.DEFAULT_SPHERE_HITS
    _check(_scene("default"), rays, 1, want, "default trianglesOnly")


@pytest.mark.parametrize("name", tr.EXTRA)
def test_extra_scenes(name, gpu_available):
    """A scene without a triangle, 33 spheres, equal distances across clusters (the tie rule: the lowest reference index,
    spheres before triangles), the counts around a cluster and the layer scenes around a chunk."""
    tonly = tr.geometry(name)[2]
    got = _check(_scene(name), tr.case_rays("extra", name), tonly, tr.case_expected("extra", name), f"extra {name}")
    if name == "closing_sphere":
        assert (got["prim"] == -2).all()
    if name.startswith("ties_"):
        assert (got["prim"] == 0).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097])
def test_ray_counts_and_guards(n, gpu_available):
    """The tail: a lone live lane in a wave, partial waves and blocks.  The word after each buffer's end stays."""
    import torch

    base = tr.replay("chunks")
    rays = np.concatenate([base] * (n // len(base) + 1))[:n]
    want = tr.expected(tr.geometry("chunks")[0], None, 1, rays)
    ds, d = _scene("chunks"), _dev(rays)
    for flags in FLAGS:
        bufs = {k: torch.full((n * w + 1,), GUARD, dtype=torch.int32, device="cuda") for k, w in WORDS.items()}
        torch.cuda.synchronize()
        ds.trace_rays_async(d.data_ptr(), n, True, flags, *(bufs[k].data_ptr() for k in tr.NAMES),
                            stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k, w in WORDS.items():
            host = bufs[k].cpu().numpy().view(np.uint32)
            assert host[-1] == GUARD, f"{k}: the word after the buffer was written"
            assert np.array_equal(host[:-1], np.ascontiguousarray(want[k]).view(np.uint32).ravel()), (k, flags)


@pytest.mark.parametrize("want", [("prim",), ("depth",), ("normal",), ("albedo",), ("prim", "depth")])
def test_buffer_subsets(want, gpu_available):
    """Only the buffers asked for (the others are null: a store through one would fault) equal the four-buffer run."""
    rays, ds = tr.replay("default"), _scene("default")
    full = tr.case_expected("replay", "default")
    for flags in FLAGS:
        got = _trace(ds, rays, 0, flags, want)
        assert set(got) == set(want)
        assert tr.differing(got, full) == dict.fromkeys(want, 0)


def test_row_permutation(gpu_available):
    """Permuting the rays permutes the results: an answer does not depend on the neighbouring lanes' rays."""
    rays = np.concatenate([tr.replay("chunks"), tr.scaled("chunks", 3.0), tr.primary("chunks")])
    want = tr.expected(tr.geometry("chunks")[0], None, 1, rays)
    perm = np.random.default_rng(11).permutation(len(rays))
    for flags in FLAGS:
        got = _trace(_scene("chunks"), rays[perm], 1, flags)
        assert tr.differing(got, {k: v[perm] for k, v in want.items()}) == ZERO


@pytest.mark.parametrize("move", sorted(moving_scenes.HELPERS))
@pytest.mark.parametrize("name", ["chunks", "suze"])
def test_after_a_scene_update(name, move, gpu_available):
    """After DeviceScene.update the results are the moved triangles'; a query enqueued before the update on the same
    stream, read afterwards, is the old triangles' (it read the generation current when it was enqueued)."""
    import torch

    tris = tr.geometry(name)[0]
    moved = moving_scenes.HELPERS[move](tris)
    rays = np.concatenate([tr.replay(name), tr.primary(name)])
    before, after = tr.expected(tris, None, 1, rays), tr.expected(moved, None, 1, rays)
    assert tr.differing(before, after)["depth"] > 20, "the move must show"
    n, d = len(rays), _dev(rays)
    ds = rt.DeviceScene(tris, None)
    try:
        for flags in FLAGS:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                dev_tris = [torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).copy()).cuda() for t in (moved, tris)]
                old = {k: torch.zeros(n * w, dtype=torch.int32, device="cuda") for k, w in WORDS.items()}
                new = {k: torch.zeros(n * w, dtype=torch.int32, device="cuda") for k, w in WORDS.items()}
                st.synchronize()
                ds.trace_rays_async(d.data_ptr(), n, True, flags, *(old[k].data_ptr() for k in tr.NAMES), stream=st.cuda_stream)
                ds.update(tris=dev_tris[0], stream=st.cuda_stream)
                ds.trace_rays_async(d.data_ptr(), n, True, flags, *(new[k].data_ptr() for k in tr.NAMES), stream=st.cuda_stream)
                st.synchronize()
                shaped = lambda b: {k: b[k].cpu().numpy().view(np.float32 if k != "prim" else np.int32)  # noqa: E731
                                    .reshape((n, 3) if WORDS[k] == 3 else (n,)) for k in tr.NAMES}
                assert tr.differing(shaped(old), before) == ZERO, "the query before the update saw the new triangles"
                assert tr.differing(shaped(new), after) == ZERO
                ds.update(tris=dev_tris[1], stream=st.cuda_stream)  # back, for the other path
                st.synchronize()
        ds.update(tris=moved)  # the host path
        assert tr.differing(_trace(ds, rays, 1, 0), after) == ZERO
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


@pytest.mark.parametrize("triangles_only", [False, True])
def test_between_frames_and_passes(triangles_only, gpu_available):
    """Queries between pipelined (RTC_F_OVERLAP) frames and between the passes of a progressive frame: the frames, the
    accumulators and the RNG states are bit-identical to the run without the queries, chain_report() and an armed frame
    event are the render launches' alone, and the query results are right.  default, 64x40x4: with its sphere the
    one-lane-per-pixel kernel, trianglesOnly the split launch (whose overlapped frames are really in flight)."""
    import torch

    tris, spheres, _, cam = tr.geometry("default")
    ds = rt.DeviceScene(tris, spheres)
    scene = rt.default_scene()
    W, H = tr.SHAPE
    cfg = rt.RenderConfig(W, H, 4, 10, triangles_only)
    ocfg = rt.RenderConfig(W, H, 4, 10, triangles_only, overlap=True)
    rays = tr.replay("default")
    want = tr.expected(tris, spheres, int(triangles_only), rays)
    d = _dev(rays)
    query = lambda flags=0: ds.trace_rays(d, triangles_only, tr.NAMES, flags)  # noqa: E731
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            first = _frame(ds, scene, cam, cfg, st)
            st.synchronize()
            launches = ds.chain_report()["launches"]
            report = ds.chain_report()
            assert tr.differing(query(), want) == ZERO
            assert ds.chain_report() == report and ds.chain_report()["launches"] == launches
            # pipelined frames on the frame event, queries between them on the same stream
            f1 = _frame(ds, scene, cam, ocfg, st, event=True)
            q1 = query()
            f2 = _frame(ds, scene, cam, ocfg, st, event=True)
            q2 = query(NO_CULL)
            f3 = _frame(ds, scene, cam, ocfg, st, event=True)
            for f in (f1, f2, f3):
                f[2].synchronize()
                assert _same(first, f)
            assert tr.differing(q1, want) == tr.differing(q2, want) == ZERO
            torch.cuda.synchronize()
            # an armed frame event survives a query: the next render launch records it
            ev = torch.cuda.Event()
            ev.record(st)
            ds.set_frame_event(ev.cuda_event)
            query()
            col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            st.synchronize()
            ds.render_rows_async(scene, cam, ocfg, col.data_ptr(), None, None, st.cuda_stream)
            ev.synchronize()
            assert np.array_equal(col.cpu().numpy(), first[0].cpu().numpy()), "the frame event was not the render's"
            torch.cuda.synchronize()
            # between the passes of a progressive frame: colours, accumulator and RNG states against the run without
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
                        assert tr.differing(query(NO_CULL if k & 1 else 0), want) == ZERO
                st.synchronize()
                runs.append((col, acc, rng))
            assert _same(runs[0], runs[1]) and np.array_equal(runs[0][2].cpu().numpy(), runs[1][2].cpu().numpy())
            assert _same(first, runs[1])
    finally:
        torch.cuda.synchronize()
        ds.close()


def test_entry_points_and_inputs_agree(gpu_available):
    """rtc_trace_rays (host arrays: numpy RAY_DT and float32 [n, 6]) agrees with the asynchronous path (a torch tensor),
    and all of them with the oracle."""
    rays, ds = tr.replay("default"), _scene("default")
    want = tr.case_expected("replay", "default")
    for flags in FLAGS:
        host = ds.trace_rays(rays, False, tr.NAMES, flags)
        flat = ds.trace_rays(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6), False, tr.NAMES, flags)
        dev = _trace(ds, rays, 0, flags)
        assert tr.differing(host, want) == tr.differing(flat, want) == tr.differing(dev, want) == ZERO
        assert all(host[k].dtype == dev[k].dtype and host[k].shape == dev[k].shape for k in tr.NAMES)
    assert set(ds.trace_rays(rays[:100], True, ("depth",))) == {"depth"}


@pytest.mark.parametrize("only", tr.NAMES)
def test_host_entry_single_buffers(only, gpu_available):
    """rtc_trace_rays with one buffer asked for and the other three null (staged: no device buffer for them), 65 rays -- a
    wave and one lane, where a wrong byte count or a buffer in another's place shows -- on the default scene (the smallest
    fixture whose rays hit triangles and a sphere, so normal and albedo differ): the device-tensor entry's words."""
    rays, ds = tr.replay("default")[:65], _scene("default")
    for flags in FLAGS:
        host, dev = ds.trace_rays(rays, False, (only,), flags), _trace(ds, rays, 0, flags)
        assert set(host) == {only} and host[only].dtype == dev[only].dtype and host[only].shape == dev[only].shape
        assert np.array_equal(host[only].view(np.uint32), dev[only].view(np.uint32)), flags
    assert (dev["prim"] >= 0).any() and (dev["prim"] <= -2).any()


def test_refusals_on_a_scene(gpu_available):
    """On a real handle: an unknown flag and four null buffers are RTC_EINVAL with nothing enqueued; n == 0 is fine."""
    import torch

    ds, rays = _scene("suze"), _dev(tr.replay("suze"))
    buf = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    with pytest.raises(rt.RtcError) as ei:
        ds.trace_rays_async(rays.data_ptr(), len(rays), True, rt.RTC_F_NO_TILE_CULL, prim_ptr=buf.data_ptr())
    assert ei.value.code == rt._abi.RTC_EINVAL and "rtc_trace_rays_async" in str(ei.value)
    with pytest.raises(rt.RtcError):
        ds.trace_rays_async(rays.data_ptr(), len(rays), True, 0)
    ds.trace_rays_async(rays.data_ptr(), 0, True, 0, prim_ptr=buf.data_ptr())
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()
    assert tr.differing(_trace(ds, tr.replay("suze"), 1, 0), tr.case_expected("replay", "suze")) == ZERO
