"""rtc_trace_paths_async / rtc_trace_paths on the GPU (include/rtc.h): the radiance along caller-supplied rays
and the RNG states afterwards against the CPU oracle (tests/trace_paths_reference.py: main.c:95-100 around calcColor,
raytracing.c:262-296, with the ray given), compared as uint32 bit patterns for every ray, no tolerance, and the number of
calculateRayCollision calls exactly.  One exception, the project's standing one (tests/test_gpu_materials.py): where the
reference gives a NaN, any NaN is accepted.  Every set runs with the cluster cull and with RTC_F_NO_CLUSTER_CULL.  The
helper's tie to the reference's render loop and the sets' premises are tests/test_trace_paths_reference.py's, without a
GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import env_edge_scenes as ee
import moving_scenes
import oracle.binding as orc
import raytracingc_amd as rt
import trace_paths_reference as tp
import trace_rays_reference as tr

pytestmark = pytest.mark.gpu

NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
FLAGS = [0, NO_CULL]
GUARD = 0x5A5A5A5A
W, H = tp.SHAPE
SCENE = rt.default_scene()


@functools.lru_cache(maxsize=None)
def _scene(name):
    tris, spheres = tp.geometry(name)[:2]
    return rt.DeviceScene(tris, spheres)


def _dev(rays):
    """The rays as a float32 [n, 6] tensor on the device."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6).copy()).cuda()


def _words(a):
    """uint32 or float32 words as an int32 tensor on the device."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _query(ds, rays, seeds, spp, max_bounce, tonly, flags, scene=SCENE, **kw):
    return ds.trace_paths(_dev(rays), _words(seeds), scene, spp, max_bounce, bool(tonly), flags, segments=True, **kw)


def _bad(got, want):
    """(rays whose radiance differs, rays whose seed differs, the difference of the segment counts)."""
    return (tp.differing(got["radiance"], want[0]), int((np.asarray(got["seeds"]).view(np.uint32) != want[1]).sum()),
            got["segments"] - want[2])


def _check(ds, rays, seeds, spp, max_bounce, tonly, want, what, scene=SCENE):
    """Both paths against the expectation; returns the cull path's results."""
    first = None
    for flags in FLAGS:
        got = _query(ds, rays, seeds, spp, max_bounce, tonly, flags, scene)
        bad = _bad(got, want)
        print(f"{what} flags {flags:#x}: {len(rays)} rays, {want[2]} segments; differing radiance, seeds, segments {bad}")
        assert got["radiance"].shape == (len(rays), 3) and got["seeds"].dtype == np.uint32
        assert bad == (0, 0, 0), f"{what} flags {flags:#x}"
        first = first or got
    return first


@pytest.mark.parametrize("name", tp.CAMERA_CASES)
def test_camera_rays(name, gpu_available):
    """The 64 x 40 launch's primary rays with the pixels' seeds, spp 5, maxBounce 10: the helper's values, which are also the
    accumulator rtc_render_rows_async gives for the same scene and camera and the RNG states a single whole-frame pass of
    rtc_render_samples_async leaves."""
    import torch

    tris, spheres, tonly, cam = tp.geometry(name)
    rays = tp.camera_rays(name)
    ds = _scene(name)
    got = _check(ds, rays, tp.pixel_seeds(len(rays)), tp.SPP, tp.MAX_BOUNCE, tonly, tp.camera_expected(name), f"camera {name}")
    cfg = rt.RenderConfig(W, H, tp.SPP, tp.MAX_BOUNCE, bool(tonly))
    st = torch.cuda.current_stream().cuda_stream
    col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    ds.render_rows_async(SCENE, cam, cfg, col.data_ptr(), acc.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert tp.differing(got["radiance"], acc.cpu().numpy().reshape(-1, 3)) == 0, f"{name}: the frame's accumulator"
    acc2 = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    rng = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    ds.render_samples_async(SCENE, cam, cfg, 0, tp.SPP, col.data_ptr(), acc2.data_ptr(), rng.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert np.array_equal(got["seeds"], rng.cpu().numpy().view(np.uint32).reshape(-1)), f"{name}: the pass's RNG states"
    assert tp.differing(got["radiance"], acc2.cpu().numpy().reshape(-1, 3)) == 0


@pytest.mark.parametrize("name", tp.REPLAY_CASES)
def test_replay_rays(name, gpu_available):
    """Bounce rays the renderer really traces, from points on the surfaces, hashed seeds, spp 3."""
    tonly = tp.geometry(name)[2]
    rays = tr.replay(name)
    _check(_scene(name), rays, tp.hash_seeds(len(rays)), 3, tp.MAX_BOUNCE, tonly, tp.set_expected("replay", name),
           f"replay {name}")


@pytest.mark.parametrize("scale", [3.0, 1e4])
def test_scaled_rays(scale, gpu_available):
    """dir times 3 and 1e4: first segments beyond the cull's bound |dir|_1 <= 4 (those lanes keep every ball), bounce
    directions out of the reference's lerp."""
    rays = tr.scaled("chunks", scale)
    _check(_scene("chunks"), rays, tp.hash_seeds(len(rays)), 3, tp.MAX_BOUNCE, 1, tp.set_expected("scaled", "chunks", scale),
           f"scaled chunks x{scale}")


@pytest.mark.parametrize("tonly", [0, 1])
def test_odd_rays(tonly, gpu_available):
    """NaN, infinite, zero, tiny and huge components against the default scene, with and without its sphere, spp 2."""
    rays = tr.odd()[0]
    want = tp.set_expected("odd", "default", None, 2, tp.MAX_BOUNCE, tonly)
    _check(_scene("default"), rays, tp.hash_seeds(len(rays)), 2, tp.MAX_BOUNCE, tonly, want, f"odd tonly {tonly}")


def _async(ds, rays_t, seeds_t, n, spp, max_bounce, tonly, flags, rad, out, seg, first=0, count=None, scene=SCENE):
    import torch

    ds.trace_paths_async(scene, rays_t.data_ptr(), seeds_t.data_ptr(), n, spp, max_bounce, rad.data_ptr(), bool(tonly), flags,
                         first, count, out.data_ptr() if out is not None else 0, seg.data_ptr() if seg is not None else 0,
                         stream=torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ray_counts_and_guards(n, gpu_available):
    """The tail: a lone live lane in a wave, partial waves, more than one block.  The word after each output's end stays."""
    import torch

    tris = tp.geometry("chunks")[0]
    rays, seeds = tr.replay("chunks")[:n], tp.hash_seeds(257)[:n]
    want = tp.expected(tris, None, SCENE, 1, rays, seeds, 3, tp.MAX_BOUNCE)
    ds, d, s = _scene("chunks"), _dev(rays), _words(seeds)
    for flags in FLAGS:
        rad = torch.full((3 * n + 1,), GUARD, dtype=torch.int32, device="cuda")
        out = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
        seg = torch.tensor([0, 0, GUARD], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _async(ds, d, s, n, 3, tp.MAX_BOUNCE, 1, flags, rad, out, seg)
        torch.cuda.synchronize()
        r, o, g = (t.cpu().numpy().view(np.uint32) for t in (rad, out, seg))
        assert r[-1] == GUARD and o[-1] == GUARD and g[-1] == GUARD, "a word after a buffer was written"
        assert tp.differing(r[:-1].view(np.float32).reshape(n, 3), want[0]) == 0 and np.array_equal(o[:-1], want[1]), flags
        assert int(g[:2].view(np.uint64)[0]) == want[2]
        assert np.array_equal(s.cpu().numpy().view(np.uint32), seeds), "the caller's seeds were written"


@pytest.mark.parametrize("spp, max_bounce, name", [(1, 10, "chunks"), (2, 10, "chunks"), (7, 10, "chunks"), (3, 0, "chunks"),
                                                   (3, -2, "chunks"), (3, 1, "chunks"), (2, 100, "box_mirror")])
def test_sample_counts_and_bounces(spp, max_bounce, name, gpu_available):
    """On 64 rays.  maxBounce <= 0: the radiance is +0, the seeds are unchanged, no segment is counted."""
    tris, spheres, tonly, _ = tp.geometry(name)
    rays = (tr.replay(name) if name == "chunks" else tp.camera_rays(name))[:64]
    seeds = tp.hash_seeds(64)
    want = tp.expected(tris, spheres, SCENE, tonly, rays, seeds, spp, max_bounce)
    if max_bounce <= 0:
        assert not want[0].view(np.uint32).any() and np.array_equal(want[1], seeds) and want[2] == 0
    if max_bounce == 100:
        assert want[2] == 64 * spp * 100
    _check(_scene(name), rays, seeds, spp, max_bounce, tonly, want, f"{name} spp {spp} maxBounce {max_bounce}")


@pytest.mark.parametrize("name", ["chunks", "cbox_nonfinite"])
def test_passes_equal_one_call(name, gpu_available):
    """37 + 27 of 64 samples with the seeds in place (dSeedsOut == dSeeds) against one call of 64: radiance, seeds and the
    summed counter are identical, bit for bit, and the helper's.  cbox_nonfinite: inf and NaN are stored and reloaded."""
    import torch

    tris, spheres, tonly, _ = tp.geometry(name)
    rays = tp.camera_rays(name)[5::10]
    n = len(rays)
    seeds = tp.pixel_seeds(W * H)[5::10]
    want = tp.expected(tris, spheres, SCENE, tonly, rays, seeds, 64, tp.MAX_BOUNCE)
    if name == "cbox_nonfinite":
        assert (~np.isfinite(want[0])).any() and np.isfinite(want[0]).all(1).any()
    ds, d = _scene(name), _dev(rays)
    for flags in FLAGS:
        runs = []
        for cuts in ((64,), (37, 27)):
            s = _words(seeds)
            rad = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")  # (0xFF bytes: the first call must not read them)
            seg = torch.zeros(1, dtype=torch.int64, device="cuda")
            first = 0
            for count in cuts:
                _async(ds, d, s, n, 64, tp.MAX_BOUNCE, tonly, flags, rad, s, seg, first, count)
                first += count
            torch.cuda.synchronize()
            runs.append((rad.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint32), int(seg.cpu().numpy()[0])))
        one, two = runs
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and one[2] == two[2], flags
        assert tp.differing(one[0].view(np.float32), want[0]) == 0 and np.array_equal(one[1], want[1]) and one[2] == want[2]


def test_permutation(gpu_available):
    """Permuting rays and seeds permutes the outputs: a lane's result does not depend on its wave mates."""
    tris = tp.geometry("chunks")[0]
    rays = np.concatenate([tr.replay("chunks")[:400], tr.scaled("chunks", 3.0)[:300], tp.camera_rays("chunks")[::7]])
    seeds = tp.hash_seeds(len(rays))
    want = tp.expected(tris, None, SCENE, 1, rays, seeds, 3, tp.MAX_BOUNCE)
    perm = np.random.default_rng(11).permutation(len(rays))
    for flags in FLAGS:
        got = _query(_scene("chunks"), rays[perm], seeds[perm], 3, tp.MAX_BOUNCE, 1, flags)
        assert _bad(got, (want[0][perm], want[1][perm], want[2])) == (0, 0, 0), flags


@pytest.mark.parametrize("env", ["f0", "fm1_ineg", "fhalf_i1e30"])
def test_environment(env, gpu_available):
    """Edge environments (tests/env_edge_scenes.py: focus 0, negative focus and intensity, a huge intensity) on rays that
    miss at once -- the frame's own camera rays, along the horizon and across the sun's terminator -- and rays that bounce
    first, spp 2."""
    rec, cam = ee.edge_frames()[env]
    scene = ee.scene_struct(rec)
    tris = tp.geometry("chunks")[0]
    rays = np.concatenate([ee.primary_rays(cam, 32, 20), tp.camera_rays("chunks")[::4], tr.replay("chunks")[:300]])
    seeds = tp.hash_seeds(len(rays))
    with np.errstate(all="ignore"):
        _, _, calls, ncalls = orc.calc_path(tris, np.zeros(0, rt.SPHERE_DT), scene, 1, rays, seeds,
                                            np.full(len(rays), tp.MAX_BOUNCE, np.int32))
    last = calls[np.arange(len(rays)), ncalls - 1]["winner"]
    assert ((ncalls == 1) & (last == -1)).sum() > 300 and ((ncalls >= 2) & (last == -1)).sum() > 50
    want = tp.expected(tris, None, scene, 1, rays, seeds, 2, tp.MAX_BOUNCE)
    _check(_scene("chunks"), rays, seeds, 2, tp.MAX_BOUNCE, 1, want, f"environment {env}", scene)


@pytest.mark.parametrize("move", sorted(moving_scenes.HELPERS))
def test_after_a_scene_update(move, gpu_available):
    """After DeviceScene.update the query gives the new geometry's paths."""
    import torch

    tris = tp.geometry("chunks")[0]
    moved = moving_scenes.HELPERS[move](tris)
    rays = np.concatenate([tr.replay("chunks")[:500], tp.camera_rays("chunks")[::5]])
    seeds = tp.hash_seeds(len(rays))
    before = tp.expected(tris, None, SCENE, 1, rays, seeds, 2, tp.MAX_BOUNCE)
    after = tp.expected(moved, None, SCENE, 1, rays, seeds, 2, tp.MAX_BOUNCE)
    assert tp.differing(before[0], after[0]) > 20, "the move must show"
    ds = rt.DeviceScene(tris, None)
    try:
        _check(ds, rays, seeds, 2, tp.MAX_BOUNCE, 1, before, f"before {move}")
        ds.update(tris=moved)
        _check(ds, rays, seeds, 2, tp.MAX_BOUNCE, 1, after, f"after {move}")
    finally:
        torch.cuda.synchronize()
        ds.close()


def test_between_overlapped_frames(gpu_available):
    """A query between two RTC_F_OVERLAP frames on their stream: both frames equal their oracle, chain_report() is what
    the first frame's launch left, and the query's results are right."""
    import torch

    tris, _, _, cam = tp.geometry("default")
    cfg = rt.RenderConfig(W, H, 4, 10, True, overlap=True)
    ocol, oacc, _ = orc.render(tris, None, SCENE, cam, rt.RenderConfig(W, H, 4, 10, True).desc())
    rays = tr.replay("default")[:1000]
    seeds = tp.hash_seeds(len(rays))
    want = tp.expected(tris, None, SCENE, 1, rays, seeds, 2, tp.MAX_BOUNCE)
    ds = rt.DeviceScene(tris, None)
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d, s, n = _dev(rays), _words(seeds), len(rays)
            frames = [(torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda"),
                       torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")) for _ in range(2)]
            outs = [(torch.zeros((n, 3), dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
                     torch.zeros(1, dtype=torch.int64, device="cuda")) for _ in range(2)]
            st.synchronize()
            # nothing below waits for the device before the end: the frames are in flight around the queries
            ds.render_rows_async(SCENE, cam, cfg, frames[0][0].data_ptr(), frames[0][1].data_ptr(), None, st.cuda_stream)
            report = ds.chain_report()
            _async(ds, d, s, n, 2, tp.MAX_BOUNCE, 1, 0, *outs[0])
            assert ds.chain_report() == report
            ds.render_rows_async(SCENE, cam, cfg, frames[1][0].data_ptr(), frames[1][1].data_ptr(), None, st.cuda_stream)
            report = ds.chain_report()
            _async(ds, d, s, n, 2, tp.MAX_BOUNCE, 1, NO_CULL, *outs[1])
            assert ds.chain_report() == report
            torch.cuda.synchronize()
            for col, acc in frames:
                assert np.array_equal(col.cpu().numpy(), ocol)
                assert tp.differing(acc.cpu().numpy().reshape(-1, 3), oacc.reshape(-1, 3)) == 0
            for rad, out, seg in outs:
                got = {"radiance": rad.cpu().numpy(), "seeds": out.cpu().numpy().view(np.uint32),
                       "segments": int(seg.cpu().numpy()[0])}
                assert _bad(got, want) == (0, 0, 0)
    finally:
        torch.cuda.synchronize()
        ds.close()


def test_host_entry(gpu_available):
    """rtc_trace_paths (numpy arrays) gives what the tensor route gives, a continuation (first > 0) included; RAY_DT and
    float32 [n, 6] rays agree; the caller's arrays are left as they were."""
    import torch

    tris, spheres, tonly, _ = tp.geometry("default")
    rays = tr.replay("default")[:700]
    seeds = tp.hash_seeds(len(rays))
    ds = _scene("default")
    want = tp.expected(tris, spheres, SCENE, tonly, rays, seeds, 5, tp.MAX_BOUNCE)
    part = tp.expected(tris, spheres, SCENE, tonly, rays, seeds, 5, tp.MAX_BOUNCE, 0, 2)
    for flags in FLAGS:
        host = ds.trace_paths(rays, seeds, SCENE, 5, tp.MAX_BOUNCE, False, flags, segments=True)
        flat = ds.trace_paths(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6), seeds, SCENE, 5, tp.MAX_BOUNCE,
                              False, flags, segments=True)
        dev = _query(ds, rays, seeds, 5, tp.MAX_BOUNCE, tonly, flags)
        assert _bad(host, want) == _bad(flat, want) == _bad(dev, want) == (0, 0, 0)
        assert all(host[k].dtype == dev[k].dtype and host[k].shape == dev[k].shape for k in ("radiance", "seeds"))
        # two calls through each route: [0, 2) then [2, 5)
        h1 = ds.trace_paths(rays, seeds, SCENE, 5, tp.MAX_BOUNCE, False, flags, 0, 2, segments=True)
        assert _bad(h1, part) == (0, 0, 0)
        kept = h1["radiance"].copy()
        h2 = ds.trace_paths(rays, h1["seeds"], SCENE, 5, tp.MAX_BOUNCE, False, flags, 2, None, h1["radiance"], segments=True)
        assert np.array_equal(kept.view(np.uint32), h1["radiance"].view(np.uint32)), "the caller's radiance was written"
        d2 = ds.trace_paths(_dev(rays), _words(h1["seeds"]), SCENE, 5, tp.MAX_BOUNCE, False, flags, 2, 3,
                            _words(h1["radiance"]).view(torch.float32).reshape(-1, 3), segments=True)
        for two in (h2, d2):
            assert tp.differing(two["radiance"], want[0]) == 0 and np.array_equal(two["seeds"], want[1])
            assert h1["segments"] + two["segments"] == want[2]
    assert "segments" not in ds.trace_paths(rays[:10], seeds[:10], SCENE, 1, 1)


@pytest.mark.parametrize("with_seeds, with_segments", [(False, False), (True, False), (False, True), (True, True)])
def test_host_entry_optional_outputs(with_seeds, with_segments, gpu_available):
    """rtc_trace_paths itself (the Python method always asks for the states) continuing an accumulation (sampleFirst > 0:
    the radiance is staged in) with and without seedsOut and segments, 65 rays -- a wave and one lane -- on the default
    scene: the radiance, and the states and the count where asked for, are the device-tensor entry's for the same
    continuation; an output not asked for is left alone, the counter is added to."""
    import ctypes as C

    import torch

    ptr = rt._abi._ptr
    rays, seeds, ds = np.ascontiguousarray(tr.replay("default")[:65]), tp.hash_seeds(65), _scene("default")
    for flags in FLAGS:
        first = ds.trace_paths(_dev(rays), _words(seeds), SCENE, 5, tp.MAX_BOUNCE, False, flags, 0, 2)
        dev = ds.trace_paths(_dev(rays), _words(first["seeds"]), SCENE, 5, tp.MAX_BOUNCE, False, flags, 2, 3,
                             _words(first["radiance"]).view(torch.float32).reshape(-1, 3), segments=True)
        rad, sd = first["radiance"].copy(), np.ascontiguousarray(first["seeds"], np.uint32)
        out, seg = np.full(65, GUARD, np.uint32), C.c_ulonglong(1000)
        d = rt.RtcPathDesc(5, tp.MAX_BOUNCE, 0, flags, 2, 3)
        rc = rt.lib().rtc_trace_paths(ds._h, C.byref(SCENE), ptr(rays), ptr(sd), 65, C.byref(d), ptr(rad),
                                      ptr(out) if with_seeds else None,
                                      C.cast(C.pointer(seg), C.c_void_p) if with_segments else None)
        assert rc == 0, flags
        assert np.array_equal(rad.view(np.uint32), dev["radiance"].view(np.uint32)), flags
        assert np.array_equal(out, dev["seeds"] if with_seeds else np.full(65, GUARD, np.uint32)), flags
        assert seg.value == 1000 + (dev["segments"] if with_segments else 0), flags
        assert np.array_equal(sd, first["seeds"]) and dev["segments"] > 0
