"""Passes over a list of pixels on the GPU (rtc_render_pixels_async).  Every comparison is zero differing
words, no tolerance, first against rtc_render_samples_async -- the whole passes that tests/test_gpu_progressive.py pins to
the CPU reference -- and at each case's end against tests/pixel_pass_reference.py (no code under test in its loop) or
oracle.render: a listed pixel holds the accumulator, the RNG state and the Color of whole passes over the same samples, and
every other byte of the three buffers is what it was.

Every buffer is followed by 64 guard bytes that every case checks, and is filled with 0xFF bytes before its first pass.
64x40 frames unless stated (never height 1), spp 12, maxBounce 4, both kernels (a lane per pixel; RTC_F_WAVE_PER_RAY, a wave
per pixel).  The lists come from pixel_pass_reference by rule; tests/test_pixel_pass_reference.py shows they hold pixels that
never hit, that hit once and that hit several times in a sample, wherever the frame has them."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import pixel_pass_reference as ppr
import progressive_reference as pr
import raytracingc_amd as rt
from chain_path_scenes import SCENES as PATH_SCENES
from moving_scenes import shift

pytestmark = pytest.mark.gpu

W, H, SPP, MAX_BOUNCE = 64, 40, 12, 4
KERNELS = {"lane": 0, "wave": rt.RTC_F_WAVE_PER_RAY}
NO_CULL = rt.RTC_F_NO_CLUSTER_CULL
GUARD, GUARD_BYTE = 64, 0xA5
LIST_SIZES = (1, 63, 64, 65, 129)
SCENES = pr.SCENE_NAMES + ("chunks_open5",)
NO_CULL_SCENES = ("fsuzane", "chunks_open5")


def _cfg(name, w=W, h=H, spp=SPP, mb=MAX_BOUNCE, **kw):
    return rt.RenderConfig(w, h, spp, mb, bool(pr.geometry(name)[4]), **kw)


@functools.lru_cache(maxsize=None)
def _device_scene(name):
    tris, sph = pr.geometry(name)[:2]
    return rt.DeviceScene(tris, sph)


@functools.lru_cache(maxsize=None)
def _reference(name, w=W, h=H, row_start=0, row_stride=1, row_band=0):
    """(per-sample states, classes) of the scene's frame: computed once, shared, read-only."""
    tris, sph, scene, cam, _ = pr.geometry(name)
    d = _cfg(name, w, h, row_start=row_start, row_stride=row_stride, row_band=row_band).desc()
    cache = {}
    return ppr.per_sample(tris, sph, scene, cam, d, cache), ppr.classes(pr.hits_per_sample(tris, sph, scene, cam, d, cache))


class Buffers:
    """A frame's three device buffers, each followed by guard bytes, and one u64 counter."""

    def __init__(self, cfg, fill=0xFF):
        import torch

        self.n = cfg.rows() * cfg.width
        self.raw = {k: torch.full((self.n * b + GUARD,), fill, dtype=torch.uint8, device="cuda")
                    for k, b in (("col", 3), ("acc", 12), ("rng", 4))}
        for t in self.raw.values():
            t[-GUARD:] = GUARD_BYTE
        self.seg = torch.zeros(1, dtype=torch.int64, device="cuda")

    def ptr(self, k):
        return self.raw[k].data_ptr()

    def clone(self):
        import torch

        other = object.__new__(Buffers)
        other.n, other.raw, other.seg = self.n, {k: t.clone() for k, t in self.raw.items()}, torch.zeros_like(self.seg)
        return other

    def host(self):
        """(accumulator words [n, 3], states [n], Color bytes [n, 3]); the guard bytes are checked on the way."""
        import torch

        torch.cuda.synchronize()
        raw = {k: t.cpu().numpy() for k, t in self.raw.items()}
        for k, a in raw.items():
            assert (a[-GUARD:] == GUARD_BYTE).all(), f"the guard bytes after the {k} buffer changed"
        return (raw["acc"][:-GUARD].view(np.uint32).reshape(self.n, 3), raw["rng"][:-GUARD].view(np.uint32),
                raw["col"][:-GUARD].reshape(self.n, 3))


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _whole(ds, scene, cam, cfg, first, count, b, counters=None):
    ds.render_samples_async(scene, cam, cfg, first, count, b.ptr("col"), b.ptr("acc"), b.ptr("rng"),
                            counters.data_ptr() if counters is not None else None, _stream())


def _pixels(ds, scene, cam, cfg, first, count, lst, b, flags=0, colors=True, segments=True):
    import torch

    dev = torch.from_numpy(np.ascontiguousarray(lst, np.uint32).view(np.int32)).cuda()
    ds.render_pixels_async(scene, cam, cfg, first, count, dev.data_ptr(), len(lst), b.ptr("acc"), b.ptr("rng"),
                           b.ptr("col") if colors else 0, b.seg.data_ptr() if segments else None, flags, _stream())
    torch.cuda.synchronize()
    return dev


def _differ(got, want, who=None):
    """differing (accumulator words, states, Color bytes) between two host triples, over the pixels `who` (None: all)"""
    s = slice(None) if who is None else who
    return tuple(int((g[s] != w[s]).sum()) for g, w in zip(got, want))


def _lists(cls, n):
    out = {f"mixed{k}": ppr.mixed_list(cls, k) for k in LIST_SIZES}
    out["every"] = ppr.every_pixel(n)
    return out


# ---- 1. equivalence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_a_pixel_pass_equals_the_whole_pass_on_its_pixels(name, gpu_available):
    """Whole passes [0, 5), then a pixel pass [5, 12): the listed pixels are the whole-pass frame [0, 12)'s, the others
    hold the state after 5 byte for byte, Color included; over every pixel the counter is the whole pass's counter [0]."""
    import torch

    _, _, scene, cam, _ = pr.geometry(name)
    states, cls = _reference(name)
    cfg, ds = _cfg(name), _device_scene(name)
    after5 = Buffers(cfg)
    _whole(ds, scene, cam, cfg, 0, 5, after5)
    full = after5.clone()
    counters = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda")
    _whole(ds, scene, cam, cfg, 5, 7, full, counters)
    h5, h12 = after5.host(), full.host()
    whole_calls = int(counters.cpu().numpy()[0])
    ref = ppr.Frame(states)
    ref.whole_pass(0, 5)
    assert _differ(h5, ref.buffers()) == (0, 0, 0), f"{name}: the whole pass [0, 5) against the CPU reference"
    flag_sets = [(k, f) for k, f in KERNELS.items()]
    if name in NO_CULL_SCENES:
        flag_sets += [(k + "+no_cull", f | NO_CULL) for k, f in KERNELS.items()]
    for kernel, flags in flag_sets:
        for lname, lst in _lists(cls, W * H).items():
            what = f"{name} {kernel} {lname}"
            b = after5.clone()
            _pixels(ds, scene, cam, cfg, 5, 7, lst, b, flags)
            got = b.host()
            rest = np.setdiff1d(np.arange(W * H), lst)
            bad = _differ(got, h12, lst.astype(np.int64)), _differ(got, h5, rest)
            print(f"{what}: differing words (accumulator, state, Color) listed {bad[0]}, not listed {bad[1]}")
            assert bad == ((0, 0, 0), (0, 0, 0)), what
            want = ppr.Frame(states)
            want.whole_pass(0, 5)
            calls = want.pixel_pass(5, 7, lst)
            assert _differ(got, want.buffers()) == (0, 0, 0), f"{what}: the CPU reference"
            assert int(b.seg.cpu().numpy()[0]) == calls, f"{what}: segments {int(b.seg.cpu().numpy()[0])} vs {calls}"
            if lname == "every":
                assert calls == whole_calls, f"{what}: the whole pass counted {whole_calls}"


# ---- 2. fresh start ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["fsuzane", "open5"])
def test_a_fresh_pixel_pass_reads_nothing(name, kernel, gpu_available):
    """0xFF-filled buffers and a pixel pass [0, 12): over every pixel the oracle's accumulator and frame; over a mixed list
    of 65 the listed sky pixels hold their seed and every byte that is not listed is still 0xFF."""
    tris, sph, scene, cam, _ = pr.geometry(name)
    states, cls = _reference(name)
    cfg, ds = _cfg(name), _device_scene(name)
    ocol, oacc, oseg = orc.render(tris, sph, scene, cam, cfg.desc(), threads=16)
    b = Buffers(cfg)
    _pixels(ds, scene, cam, cfg, 0, SPP, ppr.every_pixel(W * H), b, KERNELS[kernel])
    acc, rng, col = b.host()
    assert int((acc != oacc.reshape(-1, 3).view(np.uint32)).sum()) == 0 and np.array_equal(col, ocol.reshape(-1, 3))
    assert np.array_equal(rng, states[1][SPP]) and int(b.seg.cpu().numpy()[0]) == oseg
    lst = ppr.mixed_list(cls, 65)
    b = Buffers(cfg)
    _pixels(ds, scene, cam, cfg, 0, SPP, lst, b, KERNELS[kernel])
    got = b.host()
    want = ppr.Frame(states)
    want.pixel_pass(0, SPP, lst)
    assert _differ(got, want.buffers()) == (0, 0, 0)
    rest = np.setdiff1d(np.arange(W * H), lst)
    assert all((a[rest] == (0xFF if a.dtype == np.uint8 else 0xFFFFFFFF)).all() for a in got)
    sky = np.intersect1d(lst, cls[0])
    assert len(sky) >= 8 and np.array_equal(got[1][sky], pr.seeds(cfg.desc())[sky])
    # without a Color buffer: the same accumulator and states, no Color byte written
    b = Buffers(cfg)
    _pixels(ds, scene, cam, cfg, 0, SPP, lst, b, KERNELS[kernel], colors=False, segments=False)
    nocol = b.host()
    assert _differ(nocol[:2], got[:2]) == (0, 0) and (nocol[2] == 0xFF).all()


# ---- 3. row selection and odd sizes -----------------------------------------------------------------------------------
SHAPES = {"rows_1_3": dict(row_start=1, row_stride=3), "bands_8_2": dict(row_band=8, row_stride=2),
          "37x24": dict(w=37, h=24)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_row_selections_and_odd_sizes(shape, gpu_available):
    name = "fsuzane"
    kw = SHAPES[shape]
    _, _, scene, cam, _ = pr.geometry(name)
    w, h = kw.get("w", W), kw.get("h", H)
    rows_kw = {k: v for k, v in kw.items() if k.startswith("row_")}
    states, cls = _reference(name, w, h, rows_kw.get("row_start", 0), rows_kw.get("row_stride", 1), rows_kw.get("row_band", 0))
    cfg, ds = _cfg(name, w, h, **rows_kw), _device_scene(name)
    n = cfg.rows() * w
    assert n == states[1].shape[1] and cfg.rows() > 1
    after5 = Buffers(cfg)
    _whole(ds, scene, cam, cfg, 0, 5, after5)
    full = after5.clone()
    _whole(ds, scene, cam, cfg, 5, 7, full)
    h5, h12 = after5.host(), full.host()
    last = np.uint32(n - 1)
    mixed = ppr.mixed_list(cls, 65)
    lists = {"mixed65+last": mixed if last in mixed else np.concatenate([mixed[:32], [last], mixed[32:]]).astype(np.uint32),
             "every": ppr.every_pixel(n)}
    for kernel, flags in KERNELS.items():
        for lname, lst in lists.items():
            assert last in lst
            b = after5.clone()
            _pixels(ds, scene, cam, cfg, 5, 7, lst, b, flags)
            got = b.host()
            rest = np.setdiff1d(np.arange(n), lst)
            what = f"{shape} {kernel} {lname}"
            assert (_differ(got, h12, lst.astype(np.int64)), _differ(got, h5, rest)) == ((0, 0, 0), (0, 0, 0)), what
            want = ppr.Frame(states)
            want.whole_pass(0, 5)
            want.pixel_pass(5, 7, lst)
            assert _differ(got, want.buffers()) == (0, 0, 0), f"{what}: the CPU reference"


# ---- 4. out-of-range indices ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_out_of_range_indices_are_skipped(kernel, gpu_available):
    """A list interleaved with rows * W, rows * W + 63 and 0xffffffff: the same buffers as without them, and the guard bytes
    after each buffer unchanged (Buffers.host checks them)."""
    name = "chunks"
    _, _, scene, cam, _ = pr.geometry(name)
    states, cls = _reference(name)
    cfg, ds = _cfg(name), _device_scene(name)
    n = W * H
    after5 = Buffers(cfg)
    _whole(ds, scene, cam, cfg, 0, 5, after5)
    lst = ppr.mixed_list(cls, 129)
    stale = np.empty(2 * len(lst), np.uint32)
    stale[0::2] = lst
    stale[1::2] = np.resize(np.array([n, n + 63, 0xFFFFFFFF], np.uint32), len(lst))
    clean, dirty = after5.clone(), after5.clone()
    _pixels(ds, scene, cam, cfg, 5, 7, lst, clean, KERNELS[kernel])
    _pixels(ds, scene, cam, cfg, 5, 7, stale, dirty, KERNELS[kernel])
    got = dirty.host()
    assert _differ(got, clean.host()) == (0, 0, 0)
    assert int(dirty.seg.cpu().numpy()[0]) == int(clean.seg.cpu().numpy()[0])
    want = ppr.Frame(states)
    want.whole_pass(0, 5)
    want.pixel_pass(5, 7, stale)
    assert _differ(got, want.buffers()) == (0, 0, 0)
    # nothing but indices out of range: nothing changes
    none = after5.clone()
    _pixels(ds, scene, cam, cfg, 5, 7, stale[1::2], none, KERNELS[kernel])
    assert _differ(none.host(), after5.host()) == (0, 0, 0) and int(none.seg.cpu().numpy()[0]) == 0


# ---- 5. the wave kernel's windows -------------------------------------------------------------------------------------
WINDOW_CASES = [("box_gloss", 1), ("box_gloss", 2), ("box_mirror", 63), ("box_mirror", 64), ("box_mirror", 65)]
WINDOW_COUNTS = (1, 2, 3, 5, 63, 64, 65, 130)


@pytest.mark.parametrize("scene_name,mb", WINDOW_CASES, ids=[f"{s}_mb{m}" for s, m in WINDOW_CASES])
def test_window_boundaries(scene_name, mb, gpu_available):
    """Every sample makes exactly maxBounce hits: a whole pass [0, 1), then pixel passes of 1 .. 130 samples from there --
    counts on both sides of one 64-lane window, and hit counts on both sides of it.  Both kernels and the whole pass of
    the same range leave the same words; the last count completes the frame: oracle.render's."""
    tris, cam, _ = PATH_SCENES[scene_name]
    scene = rt.default_scene()
    w, h, spp = 16, 8, 131
    cfg = rt.RenderConfig(w, h, spp, mb, True)
    ds = rt.DeviceScene(tris, None)
    try:
        first = Buffers(cfg)
        _whole(ds, scene, cam, cfg, 0, 1, first)
        every = ppr.every_pixel(w * h)
        for count in WINDOW_COUNTS:
            whole, lane, wave = first.clone(), first.clone(), first.clone()
            _whole(ds, scene, cam, cfg, 1, count, whole)
            _pixels(ds, scene, cam, cfg, 1, count, every, lane, 0)
            _pixels(ds, scene, cam, cfg, 1, count, every, wave, rt.RTC_F_WAVE_PER_RAY)
            hw, hl, hv = whole.host(), lane.host(), wave.host()
            what = f"{scene_name} maxBounce {mb}, {count} samples"
            assert _differ(hl, hw) == (0, 0, 0), f"{what}: the lane kernel against the whole pass"
            assert _differ(hv, hw) == (0, 0, 0), f"{what}: the wave kernel against the whole pass"
            assert int(lane.seg.cpu().numpy()[0]) == int(wave.seg.cpu().numpy()[0]) >= w * h * count
        ocol, oacc, _ = orc.render(tris, None, scene, cam, cfg.desc(), threads=16)
        assert int((hv[0] != oacc.reshape(-1, 3).view(np.uint32)).sum()) == 0 and np.array_equal(hv[2], ocol.reshape(-1, 3))
    finally:
        ds.close()


# ---- 6. an adaptive frame ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_render_adaptive(kernel, gpu_available):
    """render_adaptive with three shrinking selections: every pixel's accumulator, state and Color are the reference's
    after that pixel's own number of samples, and `samples` says that number."""
    name = "open5"
    tris, sph, scene, cam, _ = pr.geometry(name)
    states, cls = _reference(name)
    cfg = _cfg(name)
    picks = [ppr.mixed_list(cls, 129)]
    picks += [picks[0][:64], picks[0][:21]]
    asked = []

    def select(done, colors, accum, samples):
        assert colors.shape == (H, W, 3) and accum.shape == (H, W, 3) and samples.shape == (H, W)
        asked.append(done)
        return picks[len(asked) - 1]

    ds = rt.DeviceScene(tris, sph)
    try:
        ref = ppr.Frame(states, fill=0)
        out = []
        for k, (done, col, acc, samples) in enumerate(ds.render_adaptive(scene, cam, cfg, [3, 4, 3, 2], select,
                                                                          flags=KERNELS[kernel])):
            if k == 0:
                ref.whole_pass(0, 3)
            else:
                ref.pixel_pass(done - [4, 3, 2][k - 1], [4, 3, 2][k - 1], picks[k - 1])
            racc, _, rcol = ref.buffers()
            assert np.array_equal(samples.reshape(-1), ref.samples) and samples.dtype == np.int32
            assert int((acc.reshape(-1, 3).view(np.uint32) != racc).sum()) == 0 and np.array_equal(col.reshape(-1, 3), rcol)
            out.append(done)
        assert out == [3, 7, 10, 12] and asked == [3, 7, 10]
        assert sorted(np.unique(ref.samples).tolist()) == [3, 7, 10, 12]
        # an empty selection ends the frame; a selection that is no subset of the previous pass is refused
        assert [d for d, *_ in ds.render_adaptive(scene, cam, cfg, [3, 4], lambda *a: [])] == [3]
        sels = iter([picks[0][:8], picks[0][4:12]])
        gen = ds.render_adaptive(scene, cam, cfg, [3, 4, 5], lambda *a: next(sels))
        assert next(gen)[0] == 3 and next(gen)[0] == 7
        with pytest.raises(ValueError):
            next(gen)
    finally:
        ds.close()


# ---- 7. after an update -----------------------------------------------------------------------------------------------
def test_a_pixel_pass_after_an_update_renders_the_new_geometry(gpu_available):
    import torch

    name = "fsuzane"
    tris, _, scene, cam, _ = pr.geometry(name)
    moved = shift(tris)
    cfg = _cfg(name)
    d = cfg.desc()
    old = orc.render(tris, None, scene, cam, d, threads=16)
    new = orc.render(moved, None, scene, cam, d, threads=16)
    assert int((old[0] != new[0]).any(-1).sum()) >= 32, "the move shows in the frame"
    ds = rt.DeviceScene(tris, None)
    try:
        stale = Buffers(cfg)
        _whole(ds, scene, cam, cfg, 0, SPP, stale)  # (a frame of the old geometry, so that the update has a launch to follow)
        ds.update(tris=moved)
        after5 = Buffers(cfg)
        _whole(ds, scene, cam, cfg, 0, 5, after5)
        for kernel, flags in KERNELS.items():
            b = after5.clone()
            _pixels(ds, scene, cam, cfg, 5, 7, ppr.every_pixel(W * H), b, flags)
            whole = after5.clone()
            _whole(ds, scene, cam, cfg, 5, 7, whole)
            got = b.host()
            assert _differ(got, whole.host()) == (0, 0, 0), kernel
            assert int((got[0] != new[1].reshape(-1, 3).view(np.uint32)).sum()) == 0, f"{kernel}: the oracle's moved frame"
            assert np.array_equal(got[2], new[0].reshape(-1, 3))
            fresh = Buffers(cfg)
            _pixels(ds, scene, cam, cfg, 0, SPP, ppr.every_pixel(W * H), fresh, flags)
            assert _differ(fresh.host(), got) == (0, 0, 0), f"{kernel}: a fresh pixel pass"
            assert int(fresh.seg.cpu().numpy()[0]) == new[2]
        torch.cuda.synchronize()
    finally:
        ds.close()


# ---- 8. it leaves the scene alone -------------------------------------------------------------------------------------
def test_the_scene_is_left_as_it_was(gpu_available):
    """chain_report(), draw_cache_stats() and an armed frame event are as before the call; the event is recorded by the
    next whole launch, not by the pixel pass."""
    import torch

    name = "ultracomplex"
    tris, sph, scene, cam, _ = pr.geometry(name)
    _, cls = _reference(name)
    cfg, ocfg = _cfg(name), _cfg(name, overlap=True)
    ds = rt.DeviceScene(tris, sph)
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            first = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            st.synchronize()
            ds.render_rows_async(scene, cam, cfg, first.data_ptr(), None, None, st.cuda_stream)
            b = Buffers(cfg)
            st.synchronize()
            _whole(ds, scene, cam, cfg, 0, 5, b)
            st.synchronize()
            report, stats = ds.chain_report(), ds.draw_cache_stats()
            ev = torch.cuda.Event()
            ev.record(st)  # (a torch event has no hipEvent_t before its first record)
            ds.set_frame_event(ev.cuda_event)
            for flags in KERNELS.values():
                _pixels(ds, scene, cam, cfg, 5, 7, ppr.mixed_list(cls, 129), b, flags)
            assert ds.chain_report() == report and ds.draw_cache_stats() == stats
            col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            st.synchronize()
            ds.render_rows_async(scene, cam, ocfg, col.data_ptr(), None, None, st.cuda_stream)
            ev.synchronize()
            assert np.array_equal(col.cpu().numpy(), first.cpu().numpy()), "the frame event was not the render's"
            torch.cuda.synchronize()
            assert ds.chain_report()["launches"] == report["launches"] + 1
            b.host()
    finally:
        torch.cuda.synchronize()
        ds.close()


# ---- 9. the host entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_the_host_entry_equals_the_device_entry(kernel, gpu_available):
    name = "chunks_open5"
    _, _, scene, cam, _ = pr.geometry(name)
    states, cls = _reference(name)
    cfg, ds = _cfg(name), _device_scene(name)
    lst = ppr.mixed_list(cls, 65)
    after5 = Buffers(cfg)
    _whole(ds, scene, cam, cfg, 0, 5, after5)
    dev = after5.clone()
    _pixels(ds, scene, cam, cfg, 5, 7, lst, dev, KERNELS[kernel])
    want = dev.host()
    acc, rng, col = after5.host()
    got = ds.render_pixels(scene, cam, cfg, 5, 7, lst, acc.view(np.float32).reshape(H, W, 3), rng.reshape(H, W),
                           colors=col.reshape(H, W, 3), segments=True, flags=KERNELS[kernel])
    host = (got["accum"].reshape(-1, 3).view(np.uint32), got["rng"].reshape(-1), got["colors"].reshape(-1, 3))
    assert _differ(host, want) == (0, 0, 0) and got["segments"] == int(dev.seg.cpu().numpy()[0])
    assert _differ(after5.host(), (acc, rng, col)) == (0, 0, 0), "the caller's arrays are left as they were"
    # a fresh host pass leaves the pixels that are not listed as the caller's arrays had them
    poison = (np.full((H, W, 3), np.nan, np.float32), np.full((H, W), 7, np.uint32), np.full((H, W, 3), 9, np.uint8))
    got = ds.render_pixels(scene, cam, cfg, 0, SPP, lst, poison[0], poison[1], colors=poison[2], flags=KERNELS[kernel])
    ref = ppr.Frame(states)
    ref.pixel_pass(0, SPP, lst)
    r = ref.buffers()
    who = lst.astype(np.int64)
    host = (got["accum"].reshape(-1, 3).view(np.uint32), got["rng"].reshape(-1), got["colors"].reshape(-1, 3))
    assert _differ(host, r, who) == (0, 0, 0)
    rest = np.setdiff1d(np.arange(W * H), who)
    assert np.isnan(got["accum"].reshape(-1, 3)[rest]).all() and (host[1][rest] == 7).all() and (host[2][rest] == 9).all()
    # device tensors: updated in place, the same words
    import torch

    t = after5.clone()
    n = t.n
    res = ds.render_pixels(scene, cam, cfg, 5, 7, torch.from_numpy(lst.view(np.int32)).cuda(),
                           t.raw["acc"][:12 * n].view(torch.float32), t.raw["rng"][:4 * n].view(torch.int32),
                           colors=t.raw["col"][:3 * n], segments=True, flags=KERNELS[kernel])
    assert _differ(t.host(), want) == (0, 0, 0) and res["segments"] == int(dev.seg.cpu().numpy()[0])
