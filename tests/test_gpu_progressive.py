"""Progressive passes on the GPU (rtc_render_samples_async) against the CPU reference of
tests/progressive_reference.py: after EVERY pass of every split the accumulator (as uint32 words), the per-pixel RNG state
and the Color frame equal the reference's after that many iterations of main.c:98-99 -- zero differing words, no
tolerance -- and after the last pass they equal oracle.render's frame and rtc_render_rows_async's of the same desc; the
segment counter [0] summed over the passes is the oracle's.  The three buffers are filled with 0xFF bytes before the first
pass: a first pass that read its inputs, or a sky pixel whose state was never written, would show.

64x40 frames (never height 1), spp 12 and 70 -- 70 needs more than one 64-lane window of rtc_render_chain, and its split
[3, 64, 3] puts a pass boundary inside a window -- maxBounce 4 (0 and 1 once), on the scenes of progressive_reference
(tests/test_progressive_reference.py shows they have pixels with no, one and several hits per sample) and every route that
changes a pixel kernel: the split launch with deferred and in-kernel sums, hoisted primaries, the one-lane-per-pixel
kernel, calcDebugColor, the sphere split, row and band shares (hoisted primaries with both ways of summing); each with
and without segment counters (the COUNT instantiations)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import oracle.binding as orc
import progressive_reference as pr
import raytracingc_amd as rt
from raytracingc_amd._abi import RtcSampleRange

pytestmark = pytest.mark.gpu

W, H, MAX_BOUNCE = 64, 40, 4
ROUTES = {
    "default": {}, "no_coop": dict(coop=False), "hoist": dict(hoist=True), "chain_inline": dict(chain_inline=True),
    "hoist_inline": dict(hoist=True, chain_inline=True),
    "split_spheres": dict(split_spheres=True), "debug": dict(debug_bounces=True),
    "rows_1_3": dict(row_start=1, row_stride=3), "bands_8_2": dict(row_band=8, row_stride=2),
}
SPLITS = {"12": [12], "1x12": [1] * 12, "5_1_6": [5, 1, 6], "3_64_3": [3, 64, 3]}
SPHERE_SCENES = ("default", "open5")
# every scene on every route with a boundary inside the frame and one inside a 64-lane window; the whole frame as one pass
# and one pass per sample on the default route
CASES = [(n, r, s) for n in pr.SCENE_NAMES for r in ROUTES for s in ("5_1_6", "3_64_3")
         if r != "split_spheres" or n in SPHERE_SCENES]
CASES += [(n, "default", s) for n in pr.SCENE_NAMES for s in ("12", "1x12")]
# several chunks and spheres in one pass (rtc_render_chain<MULTI, COUNT or not, ..., SPHERES, RESUME>: no scene above is both)
CASES += [("chunks_open5", "split_spheres", "5_1_6")]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cfg(name, spp, route, mb=MAX_BOUNCE):
    return rt.RenderConfig(W, H, spp, mb, bool(pr.geometry(name)[4]), **ROUTES[route])


@functools.lru_cache(maxsize=None)
def _device_scene(name):
    tris, sph = pr.geometry(name)[:2]
    return rt.DeviceScene(tris, sph)


@functools.lru_cache(maxsize=None)
def _sample_cache(name, rows_key):
    return {}


@functools.lru_cache(maxsize=None)
def _reference(name, spp, mb, debug, row_start, row_stride, row_band, split):
    """The reference's state after every pass of the split, and the oracle's frame: computed once, shared, read-only."""
    tris, sph, scene, cam, tonly = pr.geometry(name)
    cfg = rt.RenderConfig(W, H, spp, mb, bool(tonly), debug_bounces=debug, row_start=row_start, row_stride=row_stride,
                          row_band=row_band)
    d = cfg.desc()
    ch = pr.chain(tris, sph, scene, cam, d, list(split), _sample_cache(name, (row_start, row_stride, row_band)))
    ocol, oacc, oseg = orc.render(tris, sph, scene, cam, d, threads=16)
    for t in ch:
        for a in t[1:4]:
            a.setflags(write=False)
    return ch, ocol, oacc, oseg


def _ref(name, cfg, split):
    return _reference(name, cfg.spp, cfg.max_bounce, cfg.debug_bounces, cfg.row_start, cfg.row_stride, cfg.row_band,
                      tuple(split))


def _poisoned(cfg):
    import torch

    rows = cfg.rows()
    col = torch.full((rows, cfg.width, 3), 0xFF, dtype=torch.uint8, device="cuda")
    acc = torch.full((rows, cfg.width, 3), -1, dtype=torch.int32, device="cuda")  # 0xFF bytes
    rng = torch.full((rows, cfg.width), -1, dtype=torch.int32, device="cuda")
    return col, acc, rng


def _run_passes(name, cfg, split, counters):
    """The passes of one frame, each compared with the reference; returns the final (colors, accum, rng) host arrays."""
    import torch

    _, _, scene, cam, _ = pr.geometry(name)
    ch, ocol, oacc, oseg = _ref(name, cfg, split)
    ds = _device_scene(name)
    col, acc, rng = _poisoned(cfg)
    seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
    st = torch.cuda.current_stream().cuda_stream
    done = 0
    for count, (rdone, racc, rrng, rcol, _) in zip(split, ch):
        ds.render_samples_async(scene, cam, cfg, done, count, col.data_ptr(), acc.data_ptr(), rng.data_ptr(),
                                seg.data_ptr() if counters else None, st)
        torch.cuda.synchronize()
        done += count
        assert done == rdone
        what = f"{name} {split} counters={counters} after {done}/{cfg.spp}"
        a, s, c = acc.cpu().numpy().view(np.uint32), rng.cpu().numpy().view(np.uint32), col.cpu().numpy()
        bad = int((a != _bits(racc)).sum()), int((s != rrng).sum()), int((c != rcol).sum())
        print(f"{what}: differing accumulator words {bad[0]}, states {bad[1]}, colour bytes {bad[2]}")
        assert bad == (0, 0, 0), what
    assert int((a != _bits(oacc)).sum()) == 0 and np.array_equal(c, ocol), f"{name} {split}: the oracle's frame"
    if counters:
        assert int(seg.cpu().numpy()[0]) == oseg, f"{name} {split}: segments {int(seg.cpu().numpy()[0])} vs {oseg}"
    return c, a, s


@pytest.mark.parametrize("name,route,split", CASES, ids=["-".join(c) for c in CASES])
def test_passes_match_the_reference(name, route, split, gpu_available):
    import torch

    sp = SPLITS[split]
    cfg = _cfg(name, sum(sp), route)
    for counters in (False, True):
        col, acc, _ = _run_passes(name, cfg, sp, counters)
    # the ordinary launch of the same desc
    _, _, scene, cam, _ = pr.geometry(name)
    out = torch.zeros((cfg.rows(), W, 3), dtype=torch.uint8, device="cuda")
    full = torch.zeros((cfg.rows(), W, 3), dtype=torch.float32, device="cuda")
    _device_scene(name).render_rows_async(scene, cam, cfg, out.data_ptr(), full.data_ptr(), None,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int((full.cpu().numpy().view(np.uint32) != acc).sum()) == 0 and np.array_equal(out.cpu().numpy(), col)


@pytest.mark.parametrize("mb", [0, 1])
def test_max_bounce_0_and_1(mb, gpu_available):
    """maxBounce 0: no sample draws, every state stays the seed; 1: every sample ends at its first hit."""
    cfg = _cfg("ultracomplex", 12, "default", mb)
    for counters in (False, True):
        _, _, rng = _run_passes("ultracomplex", cfg, [5, 1, 6], counters)
    if mb == 0:
        assert np.array_equal(rng.reshape(-1), pr.seeds(cfg.desc()))


def test_large_share_passes_equal_the_ordinary_launch(gpu_available):
    """A 1080p 1/4 share is the one launch shape whose sky pass runs four-wave workgroups (more than 400,000 pixels, row
    stride > 1): a frame too large for the CPU reference in a test, so two passes of one sample are compared -- accumulator
    words and Color bytes -- with rtc_render_rows_async of the same desc (which tests/test_gpu_parity.py holds to the
    oracle), and the states of the pixels that moved with the seeds."""
    import torch

    name = "ultracomplex"
    _, _, scene, cam, _ = pr.geometry(name)
    cfg = rt.RenderConfig(1920, 1080, 2, MAX_BOUNCE, True, row_start=1, row_stride=4)
    ds = _device_scene(name)
    col, acc, rng = _poisoned(cfg)
    st = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        ds.render_samples_async(scene, cam, cfg, k, 1, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None, st)
    out = torch.zeros_like(col)
    full = torch.zeros((cfg.rows(), cfg.width, 3), dtype=torch.float32, device="cuda")
    ds.render_rows_async(scene, cam, cfg, out.data_ptr(), full.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert bool((acc == full.view(torch.int32)).all()) and bool((col == out).all())
    moved = rng.cpu().numpy().view(np.uint32).reshape(-1) != pr.seeds(cfg.desc())
    assert 0 < int(moved.sum()) < moved.size // 2  # the model's pixels drew, the sky's states are their seeds


ERRORS = {
    "null_range": dict(range=None), "null_accum": dict(accum=None), "null_state": dict(rng=None),
    "first<0": dict(range=(-1, 4)), "count=0": dict(range=(4, 0)), "past_spp": dict(range=(9, 4)),
    "overlap": dict(overlap=True),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_refused_passes_write_nothing(case, gpu_available):
    import torch

    name, e = "ultracomplex", ERRORS[case]
    _, _, scene, cam, _ = pr.geometry(name)
    cfg = rt.RenderConfig(W, H, 12, MAX_BOUNCE, True, overlap=e.get("overlap", False))
    col, acc, rng = _poisoned(cfg)
    d = cfg.desc()
    rg = e.get("range", (4, 4))
    L = rt.lib()
    rc = L.rtc_render_samples_async(_device_scene(name)._h, C.byref(scene), C.byref(cam), C.byref(d),
                                    C.byref(RtcSampleRange(*rg)) if rg else None, C.c_void_p(col.data_ptr()),
                                    C.c_void_p(acc.data_ptr()) if "accum" not in e else None,
                                    C.c_void_p(rng.data_ptr()) if "rng" not in e else None, None,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == rt.RTC_EINVAL
    assert b"rtc_render_samples_async" in L.rtc_last_error()
    torch.cuda.synchronize()
    assert bool((col == 0xFF).all()) and bool((acc == -1).all()) and bool((rng == -1).all())


def test_render_progressive_and_checkpoint(tmp_path, gpu_available):
    """DeviceScene.render_progressive yields the reference's frame after every pass; a frame saved after two passes and
    restored on a new DeviceScene finishes as the oracle's."""
    name, split = "fsuzane", [5, 1, 6]
    tris, sph, scene, cam, _ = pr.geometry(name)
    cfg = _cfg(name, 12, "default")
    ch, ocol, oacc, _ = _ref(name, cfg, split)
    ds = rt.DeviceScene(tris, sph)
    gen = ds.render_progressive(scene, cam, cfg, split)
    for k in range(2):
        done, col, acc = next(gen)
        assert done == ch[k][0] and int((_bits(acc) != _bits(ch[k][1])).sum()) == 0 and np.array_equal(col, ch[k][3])
    rt.save_progress(str(tmp_path / "frame.npz"), ds.progress)
    gen.close()
    ds.close()
    state = rt.load_progress(str(tmp_path / "frame.npz"))
    assert state.samples_done == 6 and np.array_equal(state.rng, ch[1][2])
    with pytest.raises(ValueError):
        state.check(_cfg(name, 70, "default"))
    ds2 = rt.DeviceScene(tris, sph)
    out = list(ds2.render_progressive(scene, cam, cfg, [6], state=state))
    assert len(out) == 1 and out[0][0] == 12
    assert int((_bits(out[0][2]) != _bits(oacc)).sum()) == 0 and np.array_equal(out[0][1], ocol)
    assert np.array_equal(ds2.progress.rng, ch[2][2])
    ds2.close()
