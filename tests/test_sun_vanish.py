"""The sky kernel's per-pixel sun skip (rtc_device.h sun_vanishes / env_vanish_limit, round 6).

Where focus * log2(x) lies below the scene's limit the sun term of getEnvironmentLight (raytracing.c:155-158) is below half
an ulp of every colour component, so skipping it leaves the reference's value bit for bit.  CPU: the limit the library
computes (host code) against its definition, and the claim itself against the oracle's environment -- every ray the
limit admits gives the same bits as the environment without a sun.  GPU: the device's flags and the environment evaluated
with them equal the oracle's on every ray (boundary rays included)."""
from __future__ import annotations

import math
import zlib

import numpy as np
import pytest

from env_edge_scenes import M30, M60, pixel_sum

import oracle.binding as orc
import raytracingc_amd as rt
from raytracingc_amd._abi import RAY_DT, SCENE_DT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(sun, horizon, zenith, ground, focus, intensity):
    s = np.zeros(1, SCENE_DT)
    sun = np.asarray(sun, np.float64)
    sun = (sun / np.linalg.norm(sun)).astype(np.float32)
    for k, v in (("normalizedSunDirection", sun), ("skyColorHorizon", horizon), ("skyColorZenith", zenith),
                 ("groundColor", ground)):
        s[k]["x"], s[k]["y"], s[k]["z"] = v
    s["sunFocus"], s["sunIntensity"] = focus, intensity
    return s[0]


def _limit_py(s):
    """env_vanish_limit restated: H = 2^(floor(log2(m (1 - 2^-20))) - 24), L = log2(H / intensity), limit = L - 1e-5 -- and
    -inf for L < -132, where powf's absolute rounding error of a subnormal result (2^-150) is no longer below
    2^-18 H / intensity, the room the 1e-5 margin leaves."""
    f, i = float(s["sunFocus"]), float(s["sunIntensity"])
    cols = [float(s[k][c]) for k in ("groundColor", "skyColorHorizon", "skyColorZenith") for c in "xyz"]
    if not (0 < f < 3.0e38 and 0 < i < 3.0e38) or not all(2.0 ** -60 <= c <= 2.0 ** 60 for c in cols):
        return -math.inf
    e = math.floor(math.log2(min(cols) * (1 - 2.0 ** -20)))
    big_l = math.log2(2.0 ** (e - 24) / i)
    return big_l - 1e-5 if big_l >= -132 else -math.inf


def _scenes():
    d = rt.default_scene()
    yield "default", np.frombuffer(bytes(d), SCENE_DT)[0].copy()
    rng = np.random.default_rng(7)
    for k in range(10):
        cols = rng.uniform(0.02, 1.5, (3, 3)).astype(np.float32)
        if k % 3 == 0:  # a colour exactly at a power of two: the exponent bound at its tightest
            cols[rng.integers(3), rng.integers(3)] = 2.0 ** -int(rng.integers(1, 5))
        sun = rng.normal(size=3)
        sun[1] = -abs(sun[1])
        yield f"r{k}", _scene(sun, cols[0], cols[1], cols[2], float(rng.choice([4.0, 22.0, 100.0, 700.0])),
                              float(rng.choice([0.75, 3.0, 40.0, 0.01])))
    yield "zero_colour", _scene((0, -1, 0), (1, 1, 1), (0.3, 0.9, 0.0), (0.6, 0.6, 0.6), 22.0, 0.75)
    yield "neg_intensity", _scene((0, -1, 0), (1, 1, 1), (0.3, 0.9, 0.8), (0.6, 0.6, 0.6), 22.0, -0.75)
    yield "zero_focus", _scene((0, -1, 0), (1, 1, 1), (0.3, 0.9, 0.8), (0.6, 0.6, 0.6), 0.0, 0.75)
    yield from _edge_scenes()


EDGE_SUN = (0.3, -1, 0.2)


def _edge_scenes():
    """Scenes at the edge of the range env_vanish_limit accepts: tiny colours under a huge intensity, where log2(H /
    intensity) reaches the exponents at which powf's float result is subnormal (rounded absolutely, by up to 2^-150, so
    the relative bound of the proof does not hold: limits of -148 admitted rays whose sun term is exactly H), the
    neighbouring exponents where the result is still normal, and the other ends of the accepted ranges."""
    def uni(m, focus, intensity):
        return _scene(EDGE_SUN, (m, m, m), (m, m, m), (m, m, m), focus, intensity)

    yield "m60_i64_f22", uni(M60, 22.0, 2.0 ** 64)  # log2(H / I) = -148
    yield "m60_i64_f100", uni(M60, 100.0, 2.0 ** 64)
    yield "m30_i94_f22", uni(M30, 22.0, 2.0 ** 94)  # -148
    yield "m30_i71_f22", uni(M30, 22.0, 2.0 ** 71)  # -125
    yield "m30_i73_f22", uni(M30, 22.0, 2.0 ** 73)  # -127: 2^ylogx * I < H keeps powf's result above 2^-127 - ...
    yield "p60_i64_f22", uni(2.0 ** -60, 22.0, 2.0 ** 64)  # -149
    yield "big_colours", _scene(EDGE_SUN, (2.0 ** 60,) * 3, (2.0 ** 59,) * 3, (2.0 ** 60,) * 3, 22.0, 2.0 ** -100)  # +134
    yield "m60_i64_f250", uni(M60, 250.0, 2.0 ** 64)
    # mixed components: the green channel is M60 in every colour (so it is e itself, and the minimum), the others larger
    yield "m60_mixed", _scene(EDGE_SUN, (1.0, M60, 0.37), (2.0 ** -20, M60, 3.0e-9), (2.0 ** -41, M60, 1.0e-15), 22.0,
                              2.0 ** 64)
    d = np.frombuffer(bytes(rt.default_scene()), SCENE_DT)[0]
    cols = [tuple(float(d[k][c]) for c in "xyz") for k in ("skyColorHorizon", "skyColorZenith", "groundColor")]
    yield "focus_1e-3", _scene(EDGE_SUN, *cols, 1e-3, 0.75)
    yield "focus_1e30", _scene(EDGE_SUN, *cols, 1e30, 0.75)


def _rays(s, n, rng, lim):
    """Directions above the horizon (dir.y < 0 is the sun's side, raytracing.c:156) at random, plus directions whose
    focus * log2(x) lies within 0.05 of the limit (the boundary where the skip is tightest)."""
    sun = np.array([s["normalizedSunDirection"][c] for c in "xyz"], np.float64)
    d = rng.normal(size=(n, 3))
    if np.isfinite(lim):
        m = n // 2
        x = 2.0 ** ((lim + rng.uniform(-0.05, 0.01, m)) / float(s["sunFocus"]))
        x = np.clip(x, 1e-30, 1.0)
        p = rng.normal(size=(m, 3))
        p -= (p @ sun)[:, None] * sun
        p /= np.linalg.norm(p, axis=1)[:, None]
        d[:m] = x[:, None] * sun + np.sqrt(1 - x * x)[:, None] * p
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = np.zeros(n, RAY_DT)
    r["dir"]["x"], r["dir"]["y"], r["dir"]["z"] = d.astype(np.float32).T
    return r


def test_limit_matches_definition():
    for name, s in _scenes():
        lim = rt.env_vanish_limit(s)
        want = _limit_py(s)
        if math.isinf(want):
            assert lim == want, name
        else:
            assert abs(lim - want) < 1e-12, name
    d = np.frombuffer(bytes(rt.default_scene()), SCENE_DT)[0]
    # the headline scene: m = 0.263 -> H = 2^-26; skipped where 22 log2(x) < log2(2^-26 / 0.75), x < ~0.447
    assert abs(rt.env_vanish_limit(d) - (math.log2(2.0 ** -26 / 0.75) - 1e-5)) < 1e-12


def _boundary_reachable(s, lim):
    """Whether float32 values x in [2^-126, 1) exist whose focus * log2(x) lies within 0.05 below the limit -- at least
    1000 of them, so that _rays' aimed half lands there.  It does not for a limit >= 0 (every x < 1 lies far below it), for
    a focus so small that the boundary's x is below the normal floats (focus 1e-3), or so large that neighbouring floats
    are more than 0.05 apart in focus * log2(x) (focus 1e30: x = 1 - 2^-24 already gives -8.6e22)."""
    f = float(s["sunFocus"])
    if not (np.isfinite(lim) and lim < 0 and (lim - 0.05) / f > -126):
        return False
    lo, hi = np.float32(2.0 ** ((lim - 0.05) / f)), np.float32(2.0 ** (lim / f))
    return int(hi.view(np.uint32)) - int(lo.view(np.uint32)) >= 16


def _admitted(s, rays, lim):
    """(admitted, focus * log2(x)): the rays sun_vanishes admits for the limit (dir.y < 0, x a normal float below 1, and
    focus * log2(x) below the limit by a margin for numpy's log2 against glibc's)."""
    d = np.stack([rays["dir"][c] for c in "xyz"], 1).astype(np.float32)
    sun = np.array([s["normalizedSunDirection"][c] for c in "xyz"], np.float32)
    x = (d[:, 0] * sun[0] + d[:, 1] * sun[1]) + d[:, 2] * sun[2]
    ok = (d[:, 1] < 0) & (x >= 2.0 ** -126) & (x < 1)
    ylogx = np.full(len(x), np.inf)
    ylogx[ok] = float(s["sunFocus"]) * np.log2(x[ok].astype(np.float64))
    return ylogx < lim - 1e-9 * max(1.0, float(s["sunFocus"])), ylogx


@pytest.mark.parametrize("name,s", list(_scenes()), ids=lambda v: v if isinstance(v, str) else "")
def test_skip_leaves_oracle_value(name, s):
    """Every ray the limit admits (with a margin for numpy's log2 against glibc's) has the oracle's environment equal to
    the same environment without a sun (intensity +0: sun term +0), bit for bit.  The test cannot pass by admitting
    nothing: for a finite limit at least 100 admitted rays lie within 0.05 below it wherever float directions exist
    there (_boundary_reachable; otherwise the admitted rays are counted as the limit's sign demands).

    With round 6's limit (no floor on log2(H / intensity)) the scenes whose limit was -148.00001 failed here: of the
    admitted rays, m60_i64_f22 3 257 of 4 255, m60_i64_f100 7 118 of 9 537, m30_i94_f22 4 012 of 4 381, m60_i64_f250 7 911
    of 11 130 and m60_mixed 3 271 of 4 245 differed from the environment without a sun in at least one component."""
    lim = rt.env_vanish_limit(s)
    if not np.isfinite(lim):
        return
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rays = _rays(s, 20000, rng, lim)
    adm, ylogx = _admitted(s, rays, lim)
    near = int((adm & (ylogx > lim - 0.05)).sum())
    print(f"{name}: limit {lim:.5f}, {int(adm.sum())} rays admitted, {near} within 0.05 below the limit")
    if _boundary_reachable(s, lim):
        assert near >= 100
    elif lim >= 0:  # every ray towards the sun's side with a normal x < 1
        assert adm.sum() > 100 and np.array_equal(adm, np.isfinite(ylogx))
    if adm.sum() == 0:
        return
    nosun = s.copy()
    nosun["sunIntensity"] = 0.0
    a = orc.environment(rays[adm], np.repeat(s[None], adm.sum()))
    b = orc.environment(rays[adm], np.repeat(nosun[None], adm.sum()))
    bad = int((_bits(a) != _bits(b)).any(-1).sum())
    assert bad == 0, f"{name}: {bad} of {int(adm.sum())} admitted rays differ from the environment without a sun"


@pytest.mark.gpu
@pytest.mark.parametrize("name,s", list(_scenes()), ids=lambda v: v if isinstance(v, str) else "")
def test_device_skip_bit_exact(name, s, gpu_available):
    """rtc_probe_sun_vanish with the limit and gating a launch computes on the host (env_of), one scene for every lane as
    in a launch: the environment evaluated with the flags, and the sky kernel's pixel sum of environment_miss_term for spp 1
    and 3, equal the oracle's on every ray -- scenes whose limit is -inf included, where no ray may be flagged.  The rays
    run in generated order and sorted by focus * log2(x): the powf is skipped only where every lane of a wave may skip it
    (environment_t's __any), which neighbouring pixels of a frame do and shuffled rays near the limit almost never."""
    lim = rt.env_vanish_limit(s)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rays = _rays(s, 40000, rng, lim)
    for order in ("generated", "sorted"):
        if order == "sorted":
            rays = rays[np.argsort(_admitted(s, rays, lim)[1], kind="stable")]
        ref = orc.environment(rays, np.repeat(s[None], len(rays)))
        nan = np.isnan(ref)
        adm, ylogx = _admitted(s, rays, lim)
        for spp in (1, 3):
            v, out, acc = rt.sky_miss_probe(rays, s, spp)
            assert np.array_equal(np.isnan(out), nan)
            bad = int(((_bits(out) != _bits(ref)) & ~nan).any(-1).sum())
            assert bad == 0, f"{name} {order}: {bad} rays' environment differs"
            want = pixel_sum(ref, spp)
            wnan = np.isnan(want)
            assert np.array_equal(np.isnan(acc), wnan), spp
            bad = int(((_bits(acc) != _bits(want)) & ~wnan).any(-1).sum())
            assert bad == 0, f"{name} {order} spp {spp}: {bad} rays' pixel sum differs"
            if not np.isfinite(lim):
                assert v.sum() == 0
            elif _boundary_reachable(s, lim):
                assert 100 < v.sum() < len(v)
                assert (v[adm] == 1).all() and int((adm & (ylogx > lim - 0.05)).sum()) >= 100
            elif lim >= 0:
                assert v.sum() > 100
