"""rtc_denoise_host (include/rtc.h) against the numpy restatement in tests/denoise_reference.py, byte for byte,
without a GPU; the three properties of the statement (region isolation, convexity, variance reduction) on the restatement
and on the host function alike; and the filter's use on a real frame: a low-spp render of a golden scene by the CPU oracle
comes closer to a high-spp render of it."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import denoise_reference as dr
import raytracingc_amd as rt
from raytracingc_amd import _abi
from raytracingc_amd._abi import RtcDenoiseDesc

F = np.float32
SHAPES = dr.shapes(_abi.DENOISE_TILE_W, _abi.DENOISE_TILE_H)


def c_desc(d):
    return RtcDenoiseDesc(d.width, d.rows, d.iterations, d.flags, d.spp, d.normalSquarings, d.depthScale, d.colorScale,
                          d.albedoFloor)


def host(frame, d, kw, with_samples=False):
    """rt.denoise on numpy arrays (rtc_denoise_host): (out, colors)"""
    return rt.denoise(frame["accum"], dict(kw), frame["samples"] if with_samples else None,
                      d.spp if with_samples else None, c_desc(d), colors=True)


def restated(frame, d, kw, with_samples=False):
    out = dr.denoise(frame["accum"], d, frame["samples"] if with_samples else None, **kw)
    return out, dr.quantize(out)


def host_equals_restatement(frame, d, kw, with_samples, what):
    before = {k: np.array(v) for k, v in frame.items() if isinstance(v, np.ndarray)}
    got, got_colors = host(frame, d, kw, with_samples)
    want, want_colors = restated(frame, d, kw, with_samples)
    assert got.dtype == F and got.shape == (d.rows, d.width, 3) and got_colors.dtype == np.uint8
    diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(diff) == 0, (f"{what}: {len(diff)} differing words, the first at {diff[:4]}: "
                            f"{got.reshape(-1)[diff[:4]]} for {want.reshape(-1)[diff[:4]]}")
    assert np.array_equal(got_colors, want_colors), f"{what}: the Color bytes"
    for k, v in before.items():
        assert np.array_equal(v.view(np.uint8), np.asarray(frame[k]).view(np.uint8)), f"{what}: {k} changed"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_restatement(shape):
    """Every guide subset with iterations 1 .. 6 (steps up to 32, above most of these images' sizes) and, where normals
    are given, normalSquarings 0, 1 and 8 with each; sample counts on every other case."""
    w, rows = shape
    frame = dr.random_frame(w * 1000 + rows, w, rows)
    for si, subset in enumerate(dr.GUIDE_SUBSETS):
        kw, flags = dr.guide_args(frame, subset)
        cases = [(it, sq) for it in range(1, 7) for sq in ((0, 1, 8) if "normal" in kw else (si,))]
        for n, (it, sq) in enumerate(cases):
            d = dr.desc(w, rows, it, flags, frame["spp"], sq, depth_scale=0.7, color_scale=1.5, albedo_floor=0.1)
            host_equals_restatement(frame, d, kw, n % 2 == 1, f"{w}x{rows} {subset} iterations {it} squarings {sq}")


DESIGNED = dr.designed_frames()


@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_host_on_designed_values(name):
    frame, dkw = DESIGNED[name]
    flags = dkw.get("flags", 0)
    rows, w = frame["accum"].shape[:2]
    for subset in (("albedo",) if flags else ("none", "normal", "depth", "both")):
        kw, _ = dr.guide_args(frame, subset)
        for it in (1, 2, 3, 6):
            d = dr.desc(w, rows, it, spp=frame["spp"], **dkw)
            host_equals_restatement(frame, d, kw, True, f"{name} {subset} iterations {it}")
            host_equals_restatement(frame, d, kw, False, f"{name} {subset} iterations {it}, no samples")


def test_the_designed_values_do_what_they_are_for():
    """The premises, on the restatement alone: a NaN centre stays NaN and spreads to no neighbour; subnormal weights enter
    (flushed to zero the output would differ); the albedo test is strict and false for NaN; a pixel without samples is
    black; a miss pixel comes out as c * w0 / w0."""
    frame, dkw = DESIGNED["nonfinite_colours"]
    rows, w = frame["accum"].shape[:2]
    kw, _ = dr.guide_args(frame, "both")
    out = dr.denoise(frame["accum"], dr.desc(w, rows, 3, **dkw), **kw)
    bad = ~np.isfinite(frame["accum"])
    assert np.isnan(out[4, 5]).all() and np.array_equal(~np.isfinite(out), bad)
    frame, dkw = DESIGNED["subnormal_weights"]
    d = dr.desc(w, rows, 1, **dkw)
    out = dr.denoise(frame["accum"], d)
    alone = (frame["accum"] * dr.W0) / dr.W0  # what a pixel gives when no tap enters
    assert (out.view(np.uint32) != alone.view(np.uint32)).any()
    frame, dkw = DESIGNED["albedo_floor"]
    kw, flags = dr.guide_args(frame, "albedo")
    d = dr.desc(w, rows, 1, **dkw)
    a, L = frame["albedo"], dr.load(frame["accum"], d, None, frame["albedo"])
    at = a == d.albedoFloor
    assert at.any() and np.array_equal(L[at], frame["accum"][at]) and np.array_equal(L[np.isnan(a)], frame["accum"][np.isnan(a)])
    above = a == np.nextafter(d.albedoFloor, F(1))
    assert above.any() and np.array_equal(L[above], frame["accum"][above] / a[above])
    frame, dkw = DESIGNED["samples"]
    d = dr.desc(w, rows, 1, spp=frame["spp"], **dkw)
    L = dr.load(frame["accum"], d, frame["samples"])
    assert (frame["samples"] <= 0).any() and (L[frame["samples"] <= 0] == 0).all()
    assert np.array_equal(L[frame["samples"] == 1], frame["accum"][frame["samples"] == 1] * F(12))
    frame, dkw = DESIGNED["normals_squarings1"]
    kw, _ = dr.guide_args(frame, "both")
    out = dr.denoise(frame["accum"], dr.desc(w, rows, 1, **dkw), **kw)
    miss = (frame["normal"] == 0).all(-1)
    assert miss.sum() == 6 and np.array_equal(out[miss], (frame["accum"][miss] * dr.W0) / dr.W0)


# ---- the statement's properties, on the restatement and on the host function alike ------------------------------------
IMPLS = {"restatement": lambda frame, d, kw: restated(frame, d, kw)[0], "host": lambda frame, d, kw: host(frame, d, kw)[0]}


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_region_isolation(impl):
    """Two regions with orthogonal normals: changing every colour of one leaves every output byte of the other."""
    frame, left = dr.two_regions(11)
    rows, w = left.shape
    kw, _ = dr.guide_args(frame, "both")
    changed = dict(frame)
    changed["accum"] = np.where(left[..., None], frame["accum"], frame["accum"][::-1, ::-1] * F(3) + F(0.25)).astype(F)
    assert (changed["accum"][~left] != frame["accum"][~left]).all()
    for it in (1, 3, 5):
        for sq in (0, 1, 8):
            d = dr.desc(w, rows, it, normal_squarings=sq, depth_scale=0.5, color_scale=1.0)
            a, b = IMPLS[impl](frame, d, kw), IMPLS[impl](changed, d, kw)
            assert np.array_equal(a[left].view(np.uint32), b[left].view(np.uint32)), (it, sq)
            assert (a[~left] != b[~left]).any()


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_convexity(impl):
    """Finite inputs: every output lies within its region's input range, per component (a weighted mean with positive
    weights; compared in float64 with a relative slack of 1e-5 for the rounding of the sums and the quotient)."""
    frame, left = dr.two_regions(12)
    rows, w = left.shape
    for subset in ("normal", "both"):
        kw, _ = dr.guide_args(frame, subset)
        for it in (1, 2, 4, 6):
            d = dr.desc(w, rows, it, normal_squarings=2, depth_scale=0.5, color_scale=3.0)
            out = IMPLS[impl](frame, d, kw).astype(np.float64)
            for region in (left, ~left):
                src = frame["accum"][region].astype(np.float64)
                lo, hi = src.min(0), src.max(0)
                got = out[region]
                assert (got >= lo - 1e-5 * np.abs(lo)).all() and (got <= hi + 1e-5 * np.abs(hi)).all(), (subset, it)
    # without guides the whole image is one region
    d = dr.desc(w, rows, 5, color_scale=1.0)
    out = IMPLS[impl](frame, d, {}).astype(np.float64)
    src = frame["accum"].astype(np.float64).reshape(-1, 3)
    assert (out.reshape(-1, 3) >= src.min(0) * (1 - 1e-5)).all() and (out.reshape(-1, 3) <= src.max(0) * (1 + 1e-5)).all()


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_variance_reduction(impl):
    """colorScale = 0 and no guides make the iteration the plain 5 x 5 B3 kernel: on iid noise one iteration scales the
    interior variance by (sum H^2)^2 = (70 / 256)^2 = 0.0748."""
    acc = dr.noise_frame()
    size = acc.shape[0]
    d = dr.desc(size, size, 1, color_scale=0.0)
    out = IMPLS[impl]({"accum": acc}, d, {})
    ratio = float(out[2:-2, 2:-2].astype(np.float64).var() / acc[2:-2, 2:-2].astype(np.float64).var())
    print(f"{impl}: interior variance ratio {ratio:.4f} (expected {(70 / 256) ** 2:.4f})")
    assert 0.06 <= ratio <= 0.09


# ---- quality, once, on a real frame -------------------------------------------------------------------------------------
QUALITY = dict(scene="default_spheres", shape=(64, 40), low_spp=8, high_spp=1024, max_bounce=4,
               desc=dict(iterations=4, normal_squarings=5, depth_scale=1.0, color_scale=0.05, albedo_floor=0.01,
                         flags=dr.DEMODULATE))


@functools.lru_cache(maxsize=None)
def quality_frames():
    import first_hit_reference as fh
    import oracle.binding as orc

    tris, spheres, tonly, cam = fh.geometry(QUALITY["scene"])
    w, h = QUALITY["shape"]
    frames = []
    for spp in (QUALITY["low_spp"], QUALITY["high_spp"]):
        _, acc, _ = orc.render(tris, spheres, rt.default_scene(), cam,
                               _abi.RtcRenderDesc(w, h, spp, QUALITY["max_bounce"], tonly, 0, 1, 0), threads=4)
        frames.append(np.asarray(acc, F).reshape(h, w, 3))
    return frames[0], frames[1], fh.expected(QUALITY["scene"], QUALITY["shape"])


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_a_denoised_low_spp_frame_is_closer_to_the_high_spp_frame(impl):
    low, high, guides = quality_frames()
    h, w = low.shape[:2]
    d = dr.desc(w, h, **QUALITY["desc"])
    kw = {k: guides[k] for k in ("normal", "depth", "albedo")}
    out = IMPLS[impl]({"accum": low}, d, kw).astype(np.float64)
    mse_low = float(((low.astype(np.float64) - high) ** 2).mean())
    mse_out = float(((out - high) ** 2).mean())
    print(f"{impl}: MSE against {QUALITY['high_spp']} spp: {QUALITY['low_spp']} spp {mse_low:.6f}, denoised {mse_out:.6f}, "
          f"ratio {mse_out / mse_low:.3f}")
    assert np.isfinite(out).all() and mse_out < mse_low
