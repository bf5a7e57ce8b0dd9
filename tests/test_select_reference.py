"""rtc_select_pixels_host and rtc_resolve_host (include/rtc.h) against tests/select_reference.py, word for
word and without a GPU: the designed value sets, seeded random frames, input lists with invalid entries, duplicates and
descending order, the capacities around the count, the resolve against rtc_quantize of the separately scaled accumulator,
and the three conditions the end-to-end frames of tests/test_gpu_select.py rest on (on the CPU reference alone)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import pixel_pass_reference as ppr
import raytracingc_amd as rt
import select_reference as sr
from raytracingc_amd._abi import RtcSelectDesc

F = np.float32
SETS = sr.designed_sets()


def c_desc(s):
    return RtcSelectDesc(s.wAccum, s.wPrev, s.wLevel, s.floor, s.threshold, s.samplesDone)


def host_equals_reference(s, acc, prev, pixels=None, capacity=None, what=""):
    """both on (acc, prev, pixels, capacity) with samples poisoned: out, count and samples word for word; returns them"""
    npix = len(acc)
    samples = np.full(npix, -7, np.int32)
    want_out, want_count, want_samples = sr.select(acc, prev, s, pixels, capacity, samples)
    out, count = rt.select_pixels(acc, prev, c_desc(s), pixels, capacity, samples)
    assert count == want_count, f"{what}: count {count}, the reference's {want_count}"
    assert out.dtype == np.uint32 and np.array_equal(out, want_out), what
    assert np.array_equal(samples, want_samples), f"{what}: samples"
    return out, count, samples


def test_reference_on_the_designed_equalities():
    """The reference itself at the edge the issue names: d = 2, threshold = 1, l + floor = 4 is not selected; one float32
    below on the right side is, one above is not."""
    def one(name):
        s, a, p = SETS[name]
        return bool(sr.selected(a, p, s)[0])

    assert not one("equality_threshold+0") and not one("equality_weighted")
    assert [one(f"equality_threshold{k:+d}") for k in (-2, -1, 1, 2)] == [True, True, False, False]
    # (the floor one float32 below 2: the sum 2 + floor is a tie between two float32 below 4 and rounds to even, 4)
    assert [one(f"equality_floor{k:+d}") for k in (-2, -1, 1, 2)] == [True, False, False, False]
    s, a, p = SETS["nan_inputs"]
    assert sr.selected(a, p, s).tolist() == [False] * 6 + [True]
    s, a, p = SETS["inf_minus_inf"]
    assert sr.selected(a, p, s).tolist() == [False, False, False, False, False]  # (inf > inf * ... is inf > inf)
    s, a, p = SETS["dd_overflow"]
    assert sr.selected(a, p, s).all()
    s, a, p = SETS["dd_overflow_threshold_inf"]
    assert not sr.selected(a, p, s).any()
    s, a, p = SETS["level_negative"]
    assert sr.selected(a, p, s).all()
    s, a, p = SETS["level_minus_zero"]
    assert not sr.selected(a, p, s).any()
    for name in ("subnormal_right_side", "subnormal_floor"):
        s, a, p = SETS[name]
        assert sr.selected(a, p, s).all(), name  # (0 > a negative subnormal: flushed to zero it would not be)
    s, a, p = SETS["subnormal_both_sides"]
    assert sr.selected(a, p, s).tolist() == [True, False, True]
    assert len(SETS) >= 40


@pytest.mark.parametrize("name", sorted(SETS))
def test_host_on_designed_values(name):
    s, a, p = SETS[name]
    s.samplesDone = 9
    out, count, _ = host_equals_reference(s, a, p, what=name)
    assert count == int(sr.selected(a, p, s).sum())
    # the same rows through a list: reversed, each twice, an invalid entry between them
    n = len(a)
    lst = np.concatenate([np.arange(n)[::-1], [n, 0xFFFFFFFF], np.arange(n)]).astype(np.uint32)
    host_equals_reference(s, a, p, lst, what=name + " listed")


@pytest.mark.parametrize("npix", [1, 2, 63, 64, 65, 1000, 5000])
def test_host_on_random_frames(npix):
    s, acc, prev = sr.random_frame(1000 + npix, npix)
    s.samplesDone = 32
    out, count, samples = host_equals_reference(s, acc, prev, what=f"{npix} pixels")
    assert (samples == 32).all() and np.array_equal(out[:count], np.flatnonzero(sr.selected(acc, prev, s)))
    if npix >= 1000:
        assert 0.3 * npix < count < 0.7 * npix
    r = np.random.RandomState(npix)
    lists = {
        "descending": np.arange(npix)[::-1],
        "shuffled with invalid entries in the middle": np.insert(r.permutation(npix), r.randint(0, npix + 1, 5),
                                                                 [npix, npix + 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]),
        "duplicates": r.randint(0, npix, npix + 3),
        "a previous output with its tail": np.concatenate([out[:count // 2], np.full(7, 0xFFFFFFFF)]),
        "only invalid": np.full(5, npix),
        "empty": np.zeros(0, np.int64),
    }
    for what, lst in lists.items():
        lst = np.asarray(lst, np.int64).astype(np.uint32)
        got, n, stamped = host_equals_reference(s, acc, prev, lst, what=what)
        valid = lst[lst < npix]
        assert set(np.flatnonzero(stamped == 32)) == set(valid.tolist()), what
        assert n <= len(valid) and np.array_equal(got[:n], [v for v in valid if sr.selected(acc[v], prev[v], s)[0]]), what
        for cap in sorted({0, max(n - 1, 0), n, n + 1}):
            cut, m, _ = host_equals_reference(s, acc, prev, lst, cap, what=f"{what}, capacity {cap}")
            assert m == n and len(cut) == cap and np.array_equal(cut[:min(n, cap)], got[:min(n, cap)])
            assert (cut[min(n, cap):] == 0xFFFFFFFF).all()
    for cap in sorted({0, max(count - 1, 0), count, count + 1}):
        host_equals_reference(s, acc, prev, None, cap, what=f"every pixel, capacity {cap}")


def test_host_leaves_its_inputs_and_stamps_only_on_request():
    s, acc, prev = sr.random_frame(5, 300)
    a0, p0 = acc.copy(), prev.copy()
    lst = np.arange(0, 300, 3, dtype=np.uint32)
    l0 = lst.copy()
    out, count = rt.select_pixels(acc, prev, c_desc(s), lst)
    assert np.array_equal(acc.view(np.uint32), a0.view(np.uint32)) and np.array_equal(prev.view(np.uint32), p0.view(np.uint32))
    assert np.array_equal(lst, l0) and np.array_equal(out, sr.select(acc, prev, s, lst)[0])
    assert count == sr.select(acc, prev, s, lst)[1]


def quantized(v):
    """rtc_quantize (the host's floatToUint) of float32 [n, 3]"""
    return rt.vec3ToColor(np.ascontiguousarray(v, F))


@pytest.mark.parametrize("spp", [1, 12, 64, 1024])
def test_resolve_host(spp):
    r = np.random.RandomState(spp)
    npix = 4096
    acc = (r.rand(npix, 3) * r.choice([0.001, 0.05, 0.5, 1.0, 3.0], (npix, 1))).astype(F)
    odd = np.array([np.nan, -0.0, -0.25, 1.0, np.nextafter(F(1), F(0)), 2.5, np.inf, -np.inf, 0.0, 1e-40, 1 / 255, 254.5 / 255], F)
    acc[:len(odd) * 4, 0] = np.repeat(odd, 4)
    acc[len(odd) * 4:len(odd) * 8, 2] = np.repeat(odd, 4)
    samples = r.choice([0, 1, spp, spp + 1, 2 * spp + 3, max(spp // 2, 1), max(spp // 16, 1), -4], npix).astype(np.int32)
    samples[:len(odd) * 8] = np.tile(np.array([0, 1, spp, spp * 3 + 1], np.int32), len(odd) * 2)
    with np.errstate(all="ignore"):
        scale = np.where(samples > 0, F(spp) / np.maximum(samples, 1).astype(F), F(0)).astype(F)
        scaled = (acc * scale[:, None]).astype(F)
    got = rt.resolve(acc, samples, spp)
    assert got.dtype == np.uint8 and got.shape == acc.shape
    assert np.array_equal(got, quantized(scaled).reshape(acc.shape))
    assert (got[samples <= 0] == 0).all()
    same = samples == spp
    assert np.array_equal(got[same], quantized(acc[same]).reshape(-1, 3))  # (scale 1: the frame's own Color)
    a3 = acc.reshape(64, 64, 3)
    assert np.array_equal(rt.resolve(a3, samples.reshape(64, 64), spp), got.reshape(64, 64, 3))


@functools.lru_cache(maxsize=None)
def frame_accumulators(name):
    """pixel_pass_reference.per_sample's accumulators of an ADAPTIVE_FRAMES frame: computed once, shared, read-only"""
    scene_name, w, h, spp, mb = sr.ADAPTIVE_FRAMES[name][:5]
    tris, sph, scene, cam, tonly = sr.frame_geometry(scene_name)
    d = rt.RenderConfig(w, h, spp, mb, bool(tonly)).desc()
    return ppr.per_sample(tris, sph, scene, cam, d, {})[0]


@pytest.mark.parametrize("name", sorted(sr.ADAPTIVE_FRAMES))
def test_adaptive_frames_select_something(name):
    """What a GPU pass of tests/test_gpu_select.py's end-to-end frames means: on the CPU reference alone the first selection
    is non-empty and at most half the frame, a later one is a non-empty strict subset of its predecessor, the roomy
    capacity holds every selection and the truncating one is exceeded."""
    _, w, h, spp, _, passes, threshold, floor, capacity, cut = sr.ADAPTIVE_FRAMES[name]
    acc_k = frame_accumulators(name)
    npix = w * h
    lists, counts, samples, _ = sr.adaptive_frame(acc_k, spp, passes, threshold, floor, capacity)
    print(f"{name}: {npix} pixels, passes {passes}, selections {counts} (capacity {capacity})")
    assert len(counts) == len(passes) - 1 and 0 < counts[0] <= npix // 2
    assert max(counts) <= capacity
    live = [set(lst[lst < npix].tolist()) for lst in lists]
    assert any(0 < len(b) < len(a) and b < a for a, b in zip(live, live[1:]))
    assert all(b <= a for a, b in zip(live, live[1:]))
    done = np.cumsum(passes)
    assert sorted(np.unique(samples).tolist()) == sorted({int(done[1])} | {int(d) for d, l in zip(done[2:], live) if l})
    tlists, tcounts, tsamples, _ = sr.adaptive_frame(acc_k, spp, passes, threshold, floor, cut)
    print(f"{name}: truncating capacity {cut}: selections {tcounts}")
    assert tcounts[0] == counts[0] > cut > 0 and int((tlists[0] < npix).sum()) == cut
    assert np.array_equal(tlists[0], lists[0][:cut]) and tcounts[1] <= cut
