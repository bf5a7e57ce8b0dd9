"""The select and resolve kernels on the GPU (rtc_select_pixels_async, rtc_resolve_async, DeviceScene.render_adaptive_device;
DESIGN §3.20).  Every comparison is byte for byte, no tolerance, against the host statements (rtc_select_pixels_host,
rtc_resolve_host), which tests/test_select_reference.py holds to the numpy restatement.

Every device buffer the entries write is followed by guard words that every case checks -- after dOut[capacity), after
dCount, after dSamples and after the scratch's stated size -- and every input is compared with what was uploaded.  The
sizes come from the select's shape (T entries per workgroup, G tile counts per step of the scan): 1, 2, 63, 64, 65, T - 1,
T, T + 1, 2 T + 1 and G T + 1, each with and without an input list."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import pixel_pass_reference as ppr
import raytracingc_amd as rt
import select_reference as sr
from raytracingc_amd import _abi
from raytracingc_amd._abi import RtcSelectDesc

pytestmark = pytest.mark.gpu

F = np.float32
T, G = _abi.SELECT_ENTRIES_PER_GROUP, _abi.SELECT_SCAN_GROUPS
GUARD = 16  # words (bytes for byte buffers)
POISON_OUT, POISON_SAMPLES, POISON_COUNT, POISON_BYTE = 0x5A5A5A5A, -7, 0x1234567890ABCDEF, 0xA5
SIZES = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, G * T + 1)


def c_desc(s):
    return RtcSelectDesc(s.wAccum, s.wPrev, s.wLevel, s.floor, s.threshold, s.samplesDone)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared sets are read-only)


def device_equals_host(s, acc, prev, pixels=None, capacity=None, stamp=True, count=True, what=""):
    """rtc_select_pixels_async on guarded buffers against rtc_select_pixels_host: out, count and samples byte for byte, the
    guards and the inputs untouched.  Returns (out, count)."""
    import torch

    acc, prev = np.ascontiguousarray(acc, F).reshape(-1, 3), np.ascontiguousarray(prev, F).reshape(-1, 3)
    npix = len(acc)
    lst = None if pixels is None else np.ascontiguousarray(np.asarray(pixels, np.int64).astype(np.uint32))
    n = npix if lst is None else len(lst)
    capacity = n if capacity is None else capacity
    host_samples = np.full(npix, POISON_SAMPLES, np.int32)
    want_out, want_count = rt.select_pixels(acc, prev, c_desc(s), lst, capacity, host_samples if stamp else None)

    d_acc, d_prev = _dev(acc), _dev(prev)
    d_in = None if lst is None else _dev(lst.view(np.int32) if len(lst) else np.zeros(1, np.int32))
    d_out = torch.full((capacity + GUARD,), POISON_OUT, dtype=torch.int32, device="cuda")
    d_count = torch.full((1 + GUARD,), POISON_COUNT, dtype=torch.int64, device="cuda")
    d_samples = torch.full((npix + GUARD,), POISON_SAMPLES, dtype=torch.int32, device="cuda")
    nbytes = rt.select_scratch_bytes(n)
    d_scratch = torch.full((nbytes + GUARD,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    rt.select_pixels_async(d_acc.data_ptr(), d_prev.data_ptr(), npix, None if d_in is None else d_in.data_ptr(),
                           0 if lst is None else n, c_desc(s), d_out.data_ptr() if capacity else None, capacity,
                           d_count.data_ptr() if count else None, d_samples.data_ptr() if stamp else None,
                           d_scratch.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, cnt, smp, scr = (t.cpu().numpy() for t in (d_out, d_count, d_samples, d_scratch))
    assert (out[capacity:] == POISON_OUT).all(), f"{what}: the guard after dOut[capacity)"
    assert (cnt[1:] == POISON_COUNT).all(), f"{what}: the guard after dCount"
    assert (smp[npix:] == POISON_SAMPLES).all(), f"{what}: the guard after dSamples"
    assert (scr[nbytes:] == POISON_BYTE).all(), f"{what}: the guard after the scratch's stated size"
    assert np.array_equal(d_acc.cpu().numpy().view(np.uint32), acc.view(np.uint32)), f"{what}: the accumulator changed"
    assert np.array_equal(d_prev.cpu().numpy().view(np.uint32), prev.view(np.uint32)), f"{what}: the snapshot changed"
    if lst is not None and len(lst):
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), lst), f"{what}: the input list changed"
    got_count = int(cnt[0]) if count else want_count
    if count:
        assert got_count == want_count, f"{what}: count {got_count}, the host's {want_count}"
    else:
        assert cnt[0] == POISON_COUNT
    got = out[:capacity].view(np.uint32)
    diff = np.flatnonzero(got != want_out)
    assert len(diff) == 0, f"{what}: {len(diff)} differing list words, the first at {diff[:4]}: {got[diff[:4]]} for {want_out[diff[:4]]}"
    assert np.array_equal(smp[:npix], host_samples), f"{what}: the stamped samples"
    return got, got_count


def a_list(seed, n, npix):
    """n entries over npix pixels: shuffled, a few invalid ones in the middle"""
    r = np.random.RandomState(seed)
    lst = r.permutation(max(n, npix))[:n].astype(np.int64) % npix
    if n >= 3:
        lst[r.randint(0, n, max(n // 50, 1))] = r.choice([npix, npix + 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], max(n // 50, 1))
    return lst


@pytest.mark.parametrize("n", SIZES)
def test_sizes_without_a_list(n, gpu_available):
    s, acc, prev = sr.random_frame(n, n)
    s.samplesDone = 24
    out, count = device_equals_host(s, acc, prev, what=f"{n} pixels")
    assert n < 1000 or 0.3 * n < count < 0.7 * n
    for cap in sorted({0, count // 2, count, count + 1}):
        device_equals_host(s, acc, prev, None, cap, what=f"{n} pixels, capacity {cap}")


@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_a_list(n, gpu_available):
    npix = max(n // 2, 7) if n > 65 else n + 3  # (long lists hold every pixel about twice)
    s, acc, prev = sr.random_frame(n + 1, npix)
    s.samplesDone = 24
    lst = a_list(n, n, npix)
    out, count = device_equals_host(s, acc, prev, lst, what=f"a list of {n}")
    for cap in sorted({0, count // 2, count, count + 1}):
        device_equals_host(s, acc, prev, lst, cap, what=f"a list of {n}, capacity {cap}")
    # ascending, and the output of the select above with its sentinel tail as the next input
    device_equals_host(s, acc, prev, np.sort(lst), what=f"an ascending list of {n}")
    again, m = device_equals_host(s, acc, prev, out, what=f"the previous output of {n}")
    assert m == count and np.array_equal(again, out)


def pattern_frame(chosen):
    """(desc, accum, prev) whose selection is exactly the bool array `chosen`: d = 2 against 0.5 * 2, or d = 0"""
    acc = np.tile(np.array([1, 1, 0], F), (len(chosen), 1))
    prev = np.where(np.asarray(chosen)[:, None], F(0), acc).astype(F)
    return sr.desc(1, 1, 1, 0, 0.5, 3), acc, prev


def patterns(n):
    idx = np.arange(n)
    runs = np.zeros(n, bool)
    for lo, hi in ((0, 64), (128, 192), (T - 64, T), (T, T + 64), (2 * T - 1, 2 * T + 1), (2 * T + 63, 2 * T + 65),
                   (3 * T - 64, 3 * T), (3 * T + 64, n)):
        runs[lo:hi] = True
    return {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": idx % 2 == 1, "only the last": idx == n - 1,
            "only the first": idx == 0, "runs on wave and tile boundaries": runs,
            "every 64th from 63": idx % 64 == 63, "whole tiles alternating": (idx // T) % 2 == 0}


@pytest.mark.parametrize("listed", [False, True])
def test_selection_patterns_and_capacities(listed, gpu_available):
    n = 3 * T + 100
    for name, chosen in patterns(n).items():
        s, acc, prev = pattern_frame(chosen)
        lst = np.arange(n)[::-1] if listed else None  # (a descending list: the output descends too)
        want = np.flatnonzero(chosen)[::-1] if listed else np.flatnonzero(chosen)
        out, count = device_equals_host(s, acc, prev, lst, what=name)
        assert count == int(chosen.sum()) and np.array_equal(out[:count], want), name
        # cuts inside a wave, at a wave's end, inside a tile, at a tile's end, one before and one past the count, and 0
        for cap in sorted({0, 37, 64, T + 100, 2 * T, max(count - 1, 0), count + 1, n + 5}):
            cut, m = device_equals_host(s, acc, prev, lst, cap, what=f"{name}, capacity {cap}")
            assert m == count and np.array_equal(cut[:min(cap, count)], want[:min(cap, count)])
            assert (cut[min(cap, count):] == 0xFFFFFFFF).all()


def test_designed_values(gpu_available):
    """The designed sets of tests/select_reference.py, subnormals among them: the device decides as the host does."""
    wrong = []
    for name, (s, a, p) in sorted(sr.designed_sets().items()):
        s.samplesDone = 5
        n = len(a)
        lst = np.concatenate([np.arange(n)[::-1], [n, 0xFFFFFFFF], np.arange(n)])
        for what, pixels in ((name, None), (name + " listed", lst)):
            try:
                out, count = device_equals_host(s, a, p, pixels, what=what)
                want = sr.select(a, p, s, pixels)
                assert count == want[1] and np.array_equal(out, want[0]), f"{what}: the numpy restatement"
            except AssertionError as e:
                wrong.append(str(e))
    assert not wrong, "\n".join(wrong)


def test_invalid_duplicate_and_unsorted_entries(gpu_available):
    npix = 3000
    s, acc, prev = sr.random_frame(77, npix)
    s.samplesDone = 11
    r = np.random.RandomState(3)
    lists = {
        "duplicates": r.randint(0, npix, 2 * T + 77),
        "invalid entries in the middle": np.insert(np.arange(npix), r.randint(0, npix, 300), r.choice([npix, 0xFFFFFFFF, 1 << 31], 300)),
        "unsorted": r.permutation(npix),
        "only invalid": np.full(T + 5, 0xFFFFFFFF),
        "one pixel many times": np.full(200, int(np.flatnonzero(sr.selected(acc, prev, s))[0])),
    }
    for what, lst in lists.items():
        out, count = device_equals_host(s, acc, prev, lst, what=what)
        device_equals_host(s, acc, prev, lst, count // 2, what=what + ", cut")
    assert device_equals_host(s, acc, prev, lists["only invalid"], what="only invalid")[1] == 0
    assert device_equals_host(s, acc, prev, lists["one pixel many times"], what="one pixel")[1] == 200


def test_an_empty_list_is_enqueued_work(gpu_available):
    s, acc, prev = sr.random_frame(9, 500)
    for cap in (0, 1, 63, 64, T + 1, 2 * T + 9):
        out, count = device_equals_host(s, acc, prev, np.zeros(0, np.int64), cap, what=f"empty list, capacity {cap}")
        assert count == 0 and len(out) == cap and (out == 0xFFFFFFFF).all()


def test_outputs_are_optional(gpu_available):
    """A call that only stamps and counts (dOut null, capacity 0), one without samples, one without the count."""
    s, acc, prev = sr.random_frame(21, 2 * T + 300)
    s.samplesDone = 40
    lst = a_list(5, T + 31, len(acc))
    for pixels in (None, lst):
        device_equals_host(s, acc, prev, pixels, 0, what="stamp and count")
        device_equals_host(s, acc, prev, pixels, 0, count=False, what="stamp only")
        device_equals_host(s, acc, prev, pixels, 0, stamp=False, what="count only")
        device_equals_host(s, acc, prev, pixels, None, stamp=False, what="list and count")
        device_equals_host(s, acc, prev, pixels, None, stamp=False, count=False, what="list only")


def test_python_select_on_tensors(gpu_available):
    import torch

    s, acc, prev = sr.random_frame(31, 5000)
    s.samplesDone = 6
    host_samples, samples = np.zeros(5000, np.int32), torch.zeros(5000, dtype=torch.int32, device="cuda")
    want, n = rt.select_pixels(acc, prev, c_desc(s), None, 3000, host_samples)
    out, count = rt.select_pixels(_dev(acc), _dev(prev), c_desc(s), None, 3000, samples)
    assert out.is_cuda and count.is_cuda and count.dtype == torch.int64 and int(count.cpu()[0]) == n
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want) and np.array_equal(samples.cpu().numpy(), host_samples)
    want2, n2 = rt.select_pixels(acc, prev, c_desc(s), want)
    out2, count2 = rt.select_pixels(_dev(acc), _dev(prev), c_desc(s), out)
    assert int(count2.cpu()[0]) == n2 == n and np.array_equal(out2.cpu().numpy().view(np.uint32), want2)


# ---- resolve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [1, 3, 4, 5, 63, 65, 127, 129, 64 * 33 - 1, 64 * 33 + 1])
def test_resolve(npix, gpu_available):
    import torch

    spp = 48
    r = np.random.RandomState(npix)
    acc = (r.rand(npix, 3) * r.choice([0.01, 0.3, 1.0, 3.0], (npix, 1))).astype(F)
    odd = np.array([np.nan, -0.0, -0.25, 1.0, 2.5, np.inf, -np.inf, 1e-40], F)
    k = min(len(odd), npix)
    acc[:k, r.randint(3)] = odd[:k]
    samples = r.choice([0, 1, spp, spp + 1, 3 * spp, 7, -2], npix).astype(np.int32)
    want = rt.resolve(acc, samples, spp).reshape(-1)
    d_acc, d_samples = _dev(acc), _dev(samples)
    for offset in range(4):
        buf = torch.full((GUARD + 4 + 3 * npix + GUARD,), POISON_BYTE, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        at = GUARD + offset
        rt.resolve_async(d_acc.data_ptr(), d_samples.data_ptr(), npix, spp, buf.data_ptr() + at,
                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:at] == POISON_BYTE).all() and (got[at + 3 * npix:] == POISON_BYTE).all(), f"offset {offset}: the guards"
        assert np.array_equal(got[at:at + 3 * npix], want), f"offset {offset}"
    assert np.array_equal(d_acc.cpu().numpy().view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(rt.resolve(d_acc, d_samples, spp).cpu().numpy().reshape(-1), want)


# ---- a whole adaptive frame ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame_states(name):
    """pixel_pass_reference.per_sample's (accum, rng, ...) of an ADAPTIVE_FRAMES frame: computed once, shared, read-only"""
    scene_name, w, h, spp, mb = sr.ADAPTIVE_FRAMES[name][:5]
    tris, sph, scene, cam, tonly = sr.frame_geometry(scene_name)
    return ppr.per_sample(tris, sph, scene, cam, rt.RenderConfig(w, h, spp, mb, bool(tonly)).desc(), {})


def host_loop(ds, scene, cam, cfg, passes, threshold, floor, capacity, flags):
    """The existing render_adaptive with a `select` that keeps the previous accumulator and calls the host statement,
    cut at `capacity`: (accum, samples, counts) after the last pass."""
    npix = cfg.rows() * cfg.width
    done_at = np.cumsum(passes)
    state = {"prev": None, "list": None, "counts": [], "k": 0}

    def judge(accum, capacity):
        k = state["k"]
        d = rt.select_desc(cfg.spp, int(done_at[k - 1]), int(done_at[k]), threshold, floor)
        out, count = rt.select_pixels(accum, state["prev"], d, state["list"], capacity)
        state["counts"].append(count)
        return out

    def select(done, colors, accum, samples):
        if state["k"] >= 1:
            state["list"] = judge(accum, capacity)
        state["k"] += 1
        state["prev"] = accum.copy()
        return np.arange(npix) if state["list"] is None else state["list"][state["list"] < npix]

    last = None
    for last in ds.render_adaptive(scene, cam, cfg, list(passes), select, flags=flags):
        pass
    assert last[0] == done_at[-1], "a selection was empty: the frame's constants do not do what they were chosen for"
    judge(last[2], 0)
    return last[2], last[3], state["counts"]


CASES = [("ultracomplex", "roomy", "wave"), ("ultracomplex", "cut", "wave"), ("ultracomplex", "roomy", "lane"),
         ("box_diffuse_T", "roomy", "wave"), ("box_diffuse_T", "cut", "wave"), ("box_diffuse_T", "cut", "lane")]


@pytest.mark.parametrize("name,room,kernel", CASES)
def test_render_adaptive_device(name, room, kernel, gpu_available):
    """render_adaptive_device against the existing render_adaptive driven by the host statement: accum and samples, zero
    differing words; counts the host's; colors rtc_resolve_host of those; the RNG states (which render_adaptive does not
    hand out) and the accumulator also against tests/pixel_pass_reference.py at every pixel's own sample count; the scene's
    last plan and chain report as a pixel pass leaves them."""
    import torch

    scene_name, w, h, spp, mb, passes, threshold, floor, roomy, cut = sr.ADAPTIVE_FRAMES[name]
    capacity = roomy if room == "roomy" else cut
    flags = {"wave": rt.RTC_F_WAVE_PER_RAY, "lane": 0}[kernel]
    tris, sph, scene, cam, tonly = sr.frame_geometry(scene_name)
    cfg = rt.RenderConfig(w, h, spp, mb, bool(tonly))
    npix = w * h
    ds = rt.DeviceScene(tris, sph)
    try:
        # the two whole passes alone, into other buffers: what they leave in the chain report
        col0 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        acc0 = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        rng0 = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        ds.render_samples_async(scene, cam, cfg, 0, passes[0], col0.data_ptr(), acc0.data_ptr(), rng0.data_ptr(), None, st)
        ds.render_samples_async(scene, cam, cfg, passes[0], passes[1], col0.data_ptr(), acc0.data_ptr(), rng0.data_ptr(),
                                None, st)
        torch.cuda.synchronize()
        report0 = ds.chain_report()
        if kernel == "wave":
            res = ds.render_adaptive_device(scene, cam, cfg, passes, threshold, floor, capacity)  # (the default flags)
        else:
            res = ds.render_adaptive_device(scene, cam, cfg, passes, threshold, floor, capacity, flags=0)
        torch.cuda.synchronize()
        (ops, rows), report = ds.last_plan(), ds.chain_report()
        ptrs = {k: v.data_ptr() for k, v in res.items()}
        got = {k: v.cpu().numpy() for k, v in res.items()}
        accum, samples, counts = host_loop(ds, scene, cam, cfg, passes, threshold, floor, capacity, flags)
    finally:
        torch.cuda.synchronize()
        ds.close()
    print(f"{name} {room} {kernel}: capacity {capacity}, counts {counts}")
    assert got["counts"].dtype == np.int64 and got["counts"].tolist() == counts
    assert counts[0] > 0 and (room == "roomy" or counts[0] > capacity)
    assert got["samples"].dtype == np.int32 and np.array_equal(got["samples"], samples)
    assert len(np.unique(samples)) >= 3
    assert int((got["accum"].view(np.uint32) != accum.view(np.uint32)).sum()) == 0
    assert np.array_equal(got["colors"], rt.resolve(accum, samples, spp)) and got["colors"].shape == (h, w, 3)
    acc_k, rng_k = frame_states(name)[:2]
    every, flat = np.arange(npix), samples.reshape(-1)
    assert int((got["rng"].reshape(-1).view(np.uint32) != rng_k[flat, every]).sum()) == 0
    assert int((got["accum"].reshape(-1, 3).view(np.uint32) != acc_k[flat, every].view(np.uint32)).sum()) == 0
    want = sr.adaptive_frame(acc_k, spp, passes, threshold, floor, capacity)
    assert counts == want[1] and np.array_equal(flat, want[2])
    # the select and the resolve name no scene.  The scene's last plan is still the last pixel pass's: one kernel, number 17
    # (rtc_plan.h), that writes the frame's accumulator (resource 6) and states (8), reads a list (20) and no Color (5);
    # the chain report is what the two whole passes left, two launches on.
    assert ops.tolist() == [[0, 0, -1, 17]]
    named = {(int(r[1]), int(r[3])) for r in rows[:-1]}
    assert {(6, ptrs["accum"]), (8, ptrs["rng"])} <= named and 20 in {r for r, _ in named} and 5 not in {r for r, _ in named}
    assert {k: v for k, v in report.items() if k != "launches"} == {k: v for k, v in report0.items() if k != "launches"}
    assert report["launches"] == report0["launches"] + 2
