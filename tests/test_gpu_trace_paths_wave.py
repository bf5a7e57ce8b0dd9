"""RTC_F_WAVE_PER_RAY on the GPU (include/rtc.h): rtc_trace_paths_async with one wave per ray gives the radiance,
the RNG states and the number of calculateRayCollision calls of the CPU oracle (tests/trace_paths_reference.py: main.c:95-100
around calcColor, raytracing.c:262-296, with the ray given) -- compared as uint32 bit patterns for every ray, no tolerance,
and the count exactly; where the reference gives a NaN, any NaN is accepted (tests/test_gpu_materials.py's standing
exception).  Every set runs with the cluster cull and with RTC_F_NO_CLUSTER_CULL.  The sets are
tests/trace_paths_wave_sets.py's, their premises tests/test_trace_paths_wave_reference.py's, without a GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import chain_path_scenes as cps
import moving_scenes
import raytracingc_amd as rt
import trace_paths_reference as tp
import trace_rays_reference as tr
import trace_paths_wave_sets as ws

pytestmark = pytest.mark.gpu

WAVE = rt.RTC_F_WAVE_PER_RAY
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
FLAGS = [WAVE, WAVE | NO_CULL]
GUARD = 0x5A5A5A5A
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


def _query(ds, rays, seeds, spp, max_bounce, tonly, flags, **kw):
    return ds.trace_paths(_dev(rays), _words(seeds), SCENE, spp, max_bounce, bool(tonly), flags, segments=True, **kw)


def _bad(got, want):
    """(rays whose radiance differs, rays whose seed differs, the difference of the segment counts)."""
    return (tp.differing(got["radiance"], want[0]), int((np.asarray(got["seeds"]).view(np.uint32) != want[1]).sum()),
            got["segments"] - want[2])


def _check(ds, rays, seeds, spp, max_bounce, tonly, want, what, **kw):
    for flags in FLAGS:
        got = _query(ds, rays, seeds, spp, max_bounce, tonly, flags, **kw)
        bad = _bad(got, want)
        print(f"{what} flags {flags:#x}: {len(rays)} rays, {want[2]} segments; differing radiance, seeds, segments {bad}")
        assert got["radiance"].shape == (len(rays), 3) and got["seeds"].dtype == np.uint32
        assert bad == (0, 0, 0), f"{what} flags {flags:#x}"


@pytest.mark.parametrize("name", tp.CAMERA_CASES)
def test_camera_rays(name, gpu_available):
    """The 64 x 40 launch's primary rays with the pixels' seeds, spp 5, maxBounce 10: triangles only, the default box with
    its sphere, several chunks, accumulators that hold inf and NaN."""
    tonly = tp.geometry(name)[2]
    rays = tp.camera_rays(name)
    _check(_scene(name), rays, tp.pixel_seeds(len(rays)), tp.SPP, tp.MAX_BOUNCE, tonly, tp.camera_expected(name),
           f"camera {name}")


@pytest.mark.parametrize("name, spp, max_bounce", ws.WINDOW_CASES)
def test_window_edges(name, spp, max_bounce, gpu_available):
    """The next sample on the window's last lane, exactly at its end and past it; every lane a sample; a last window of one
    or two samples; mixed hit counts over several windows."""
    rays = ws.box_rays(name)
    _check(_scene(name), rays, tp.pixel_seeds(len(rays)), spp, max_bounce, 1, ws.window_expected(name, spp, max_bounce),
           f"window {name} spp {spp} maxBounce {max_bounce}")


@pytest.mark.parametrize("spp", ws.SAMPLE_COUNTS)
def test_sample_counts(spp, gpu_available):
    """Rays that hit and rays that miss in one launch, from one sample to three windows' worth."""
    rays, seeds = ws.suze_rays()
    _check(_scene("suze"), rays, seeds, spp, tp.MAX_BOUNCE, 1, ws.suze_expected(spp), f"suze[::20] spp {spp}")


@pytest.mark.parametrize("spp", ws.MISS_SPPS)
def test_miss_rays(spp, gpu_available):
    """h == 0: every sample is the first one again; spp calls per ray, the seeds as they were."""
    rays = ws.miss_rays()
    seeds = tp.hash_seeds(len(rays))
    want = ws.miss_expected(spp)
    assert want[2] == spp * len(rays) and np.array_equal(want[1], seeds)
    _check(_scene(ws.MISS_SCENE), rays, seeds, spp, tp.MAX_BOUNCE, 1, want, f"miss spp {spp}")


def test_miss_rays_continue_an_accumulation(gpu_available):
    """Samples [1, 130) onto accumulators of 1e30, inf, NaN (no add moves them: the repeated adds may stop early), -0 and 0
    (every add moves them)."""
    import torch

    rays = ws.miss_rays()
    want = ws.miss_expected(130, 1)
    acc0 = _words(ws.miss_acc0()).view(torch.float32).reshape(-1, 3)
    _check(_scene(ws.MISS_SCENE), rays, tp.hash_seeds(len(rays)), 130, tp.MAX_BOUNCE, 1, want, "miss continuation",
           first=1, count=129, radiance=acc0)


@pytest.mark.parametrize("kind, name, scale", ws.CALLER_SETS)
def test_caller_scale_rays(kind, name, scale, gpu_available):
    """Bounce rays from points on the surfaces, unnormalised directions beyond the cull's bound, spp 3."""
    rays = tr.case_rays(kind, name, scale)
    assert len(rays) <= 2560
    _check(_scene(name), rays, tp.hash_seeds(len(rays)), 3, tp.MAX_BOUNCE, 1, tp.set_expected(kind, name, scale),
           f"{kind} {name} {scale}")


@pytest.mark.parametrize("tonly", [0, 1])
def test_odd_rays(tonly, gpu_available):
    """NaN, infinite, zero, tiny and huge components against the default scene, with and without its sphere, spp 3."""
    rays = tr.odd()[0]
    want = tp.set_expected("odd", "default", None, 3, tp.MAX_BOUNCE, tonly)
    _check(_scene("default"), rays, tp.hash_seeds(len(rays)), 3, tp.MAX_BOUNCE, tonly, want, f"odd tonly {tonly}")


def _async(ds, rays_t, seeds_t, n, spp, max_bounce, tonly, flags, rad, out, seg, first=0, count=None):
    import torch

    ds.trace_paths_async(SCENE, rays_t.data_ptr(), seeds_t.data_ptr(), n, spp, max_bounce, rad.data_ptr(), bool(tonly), flags,
                         first, count, out.data_ptr() if out is not None else 0, seg.data_ptr() if seg is not None else 0,
                         stream=torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("frame", sorted(cps.PASS_FRAMES))
def test_passes_equal_one_call(frame, gpu_available):
    """37 + 27 of 64 samples with the seeds in place (dSeedsOut == dSeeds) against one call of 64 -- both passes on the wave
    kernel, the first on the lane kernel and the second on the wave kernel, and the other way round: radiance, seeds and the
    summed counter are the one call's and the helper's, bit for bit."""
    import torch

    name, rays, seeds, mb = ws.pass_frame(frame)
    n, spp = len(rays), sum(cps.PASS_SPLIT)
    want = ws.pass_expected(frame)
    ds, d = _scene(name), _dev(rays)
    for cull in (0, NO_CULL):
        runs = []
        for kernels in ((WAVE,), (WAVE, WAVE), (0, WAVE), (WAVE, 0)):
            cuts = cps.PASS_SPLIT if len(kernels) == 2 else (spp,)
            s = _words(seeds)
            rad = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")  # (0xFF bytes: the first call must not read them)
            seg = torch.zeros(1, dtype=torch.int64, device="cuda")
            first = 0
            for flags, count in zip(kernels, cuts):
                _async(ds, d, s, n, spp, mb, 1, flags | cull, rad, s, seg, first, count)
                first += count
            torch.cuda.synchronize()
            runs.append((rad.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint32), int(seg.cpu().numpy()[0])))
        one = runs[0]
        assert tp.differing(one[0].view(np.float32), want[0]) == 0 and np.array_equal(one[1], want[1]) and one[2] == want[2]
        for kernels, two in zip(("wave + wave", "lane + wave", "wave + lane"), runs[1:]):
            assert tp.differing(two[0].view(np.float32), one[0].view(np.float32)) == 0, (frame, cull, kernels)
            assert np.array_equal(one[1], two[1]) and one[2] == two[2], (frame, cull, kernels)


@pytest.mark.parametrize("n", ws.RAY_COUNTS)
def test_ray_counts_and_guards(n, gpu_available):
    """A workgroup takes four rays: a lone wave, a partial workgroup, a full one, one more.  The word after each output's
    end stays, and so do the caller's seeds."""
    import torch

    tris = tp.geometry("chunks")[0]
    rays, seeds = ws.count_rays(n)
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


@pytest.mark.parametrize("with_seeds, with_segments", [(False, True), (True, False), (False, False)])
def test_optional_outputs(with_seeds, with_segments, gpu_available):
    """dSeedsOut null, dSegments null: the rest is written as before."""
    import torch

    tris = tp.geometry("chunks")[0]
    rays, seeds = ws.edge_rays()
    want = tp.expected(tris, None, SCENE, 1, rays, seeds, 3, tp.MAX_BOUNCE)
    ds, d, s = _scene("chunks"), _dev(rays), _words(seeds)
    for flags in FLAGS:
        rad = torch.zeros((70, 3), dtype=torch.float32, device="cuda")
        out = torch.full((70,), GUARD, dtype=torch.int32, device="cuda") if with_seeds else None
        seg = torch.zeros(1, dtype=torch.int64, device="cuda") if with_segments else None
        _async(ds, d, s, 70, 3, tp.MAX_BOUNCE, 1, flags, rad, out, seg)
        torch.cuda.synchronize()
        assert tp.differing(rad.cpu().numpy(), want[0]) == 0, flags
        if with_seeds:
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want[1]), flags
        if with_segments:
            assert int(seg.cpu().numpy()[0]) == want[2], flags


@pytest.mark.parametrize("max_bounce", ws.NO_BOUNCE)
def test_no_bounce(max_bounce, gpu_available):
    """maxBounce <= 0: the radiance is +0, the seeds are unchanged, no segment is counted."""
    tris = tp.geometry("chunks")[0]
    rays, seeds = ws.edge_rays()
    want = tp.expected(tris, None, SCENE, 1, rays, seeds, 3, max_bounce)
    assert not want[0].view(np.uint32).any() and np.array_equal(want[1], seeds) and want[2] == 0
    _check(_scene("chunks"), rays, seeds, 3, max_bounce, 1, want, f"maxBounce {max_bounce}")


def test_after_a_scene_update(gpu_available):
    """After DeviceScene.update the wave query gives what the lane query of the same call gives: the new geometry's paths."""
    import torch

    tris = tp.geometry("chunks")[0]
    moved = moving_scenes.HELPERS[ws.UPDATE_MOVE](tris)
    rays, seeds = ws.update_rays()
    after = tp.expected(moved, None, SCENE, 1, rays, seeds, 2, tp.MAX_BOUNCE)
    ds = rt.DeviceScene(tris, None)
    try:
        before = _query(ds, rays, seeds, 2, tp.MAX_BOUNCE, 1, 0)
        ds.update(tris=moved)
        for cull in (0, NO_CULL):
            lane = _query(ds, rays, seeds, 2, tp.MAX_BOUNCE, 1, cull)
            wave = _query(ds, rays, seeds, 2, tp.MAX_BOUNCE, 1, WAVE | cull)
            assert _bad(wave, (lane["radiance"], lane["seeds"], lane["segments"])) == (0, 0, 0), cull
            assert _bad(wave, after) == (0, 0, 0), cull
        assert tp.differing(before["radiance"], after[0]) > 20, "the move must show"
    finally:
        torch.cuda.synchronize()
        ds.close()


def test_host_entry(gpu_available):
    """rtc_trace_paths (numpy arrays) with the flag: the helper's values."""
    tris, spheres, tonly, _ = tp.geometry("default")
    rays, seeds = ws.host_rays()
    want = tp.expected(tris, spheres, SCENE, tonly, rays, seeds, 5, tp.MAX_BOUNCE)
    host = _scene("default").trace_paths(rays, seeds, SCENE, 5, tp.MAX_BOUNCE, False, WAVE, segments=True)
    assert _bad(host, want) == (0, 0, 0)
