"""The regroup's membership without a GPU (rtc_regroup_membership_host; csrc/rtc_regroup.h): the level-by-level rank count
the device runs, in plain C++, against the upload's membership -- dword 12 of rtc_scene_records_host's clTris, made by
split_clusters' recursive std::stable_sort.  The two must agree on every input: the golden and the adversarial scenes, the
moved ones, scene sizes around every split rule's edge, and inputs designed against the ways a rank count can go wrong
(ties broken by index instead of position, the axis of two equal extents, NaN / infinite / signed-zero keys).  A numpy
restatement of the median split is the third voice on the designed inputs.  Then the refusals that need no device.  No
reference counterpart: main.c:229-243 builds its arrays once and has no clusters."""
from __future__ import annotations

import ctypes as C
import glob
import os

import numpy as np
import pytest

import raytracingc_amd as rt
from adversarial_scenes import SCENES as ADVERSARIAL
from conftest import GOLDEN, load_tris
from moving_scenes import HELPERS, VERTS, synthetic
from raytracingc_amd import _abi
from raytracingc_amd._abi import RTC_EINVAL, TRIANGLE_DT

GOLDEN_SCENES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "scenes", "*.tris")))
COUNTS = (1, 7, 8, 9, 16, 17, 24, 25, 255, 256, 257, 264, 513, 2049)


def upload_membership(tris) -> np.ndarray:
    """The upload's membership: the reference index of every clustered record, the last cluster's padding dropped."""
    return rt.scene_records_host(tris)["clTris"][:len(tris), 12].view(np.int32).copy()


def _assert_same(tris, what):
    got, want = rt.regroup_membership_host(tris), upload_membership(tris)
    assert sorted(got.tolist()) == list(range(len(tris))), f"{what}: not a permutation"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {len(tris)} positions differ from the upload's (first: {bad[:4]})"
    return got


def centroids(tris) -> np.ndarray:
    """split_clusters' centroids [n, 3] in double from the packed f32 A, AB = B - A, AC = C - A."""
    t = np.ascontiguousarray(tris, TRIANGLE_DT)
    a, b, c = (np.stack([t[v][k] for k in "xyz"], 1).astype(np.float32) for v in VERTS)
    with np.errstate(all="ignore"):
        ab, ac = (b - a).astype(np.float32), (c - a).astype(np.float32)
        return a.astype(np.float64) + (ab.astype(np.float64) + ac.astype(np.float64)) / 3.0


def median_split(cent) -> np.ndarray:
    """split_clusters restated with numpy's stable argsort (the third voice)."""
    idx = np.arange(len(cent))

    def split(lo, hi):
        n = hi - lo
        if n <= 8:
            return
        c = cent[idx[lo:hi]]
        ext = []
        for a in range(3):
            v = c[:, a][~np.isnan(c[:, a])]
            mn, mx = min([1e300] + v.tolist()), max([-1e300] + v.tolist())
            with np.errstate(all="ignore"):
                ext.append(np.float64(mx) - np.float64(mn))
        axis = 0
        for a in (1, 2):
            if ext[a] > ext[axis]:
                axis = a
        key = np.where(np.isnan(c[:, axis]), 1e300, c[:, axis])
        idx[lo:hi] = idx[lo:hi][np.argsort(key, kind="stable")]
        mid = lo + ((n + 7) // 8 + 1) // 2 * 8
        split(lo, mid)
        split(mid, hi)

    split(0, len(cent))
    return idx.astype(np.int32)


def at(points) -> np.ndarray:
    """One small triangle per point, the point its posA: centroids that differ as the points do (the same edges)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    t = np.zeros(len(p), TRIANGLE_DT)
    for k, c in enumerate("xyz"):
        t["posA"][c] = p[:, k]
        t["posB"][c] = p[:, k] + np.float32(0.25 if k == 0 else 0.0)
        t["posC"][c] = p[:, k] + np.float32(0.25 if k == 1 else 0.0)
    t["normal"]["z"] = -1.0
    return t


# ---- the scenes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_SCENES)
def test_golden_scenes(name):
    assert len(GOLDEN_SCENES) >= 17
    _assert_same(load_tris(name)[0], name)


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_scenes(name):
    _assert_same(ADVERSARIAL[name][0], name)


@pytest.mark.parametrize("helper", sorted(HELPERS))
@pytest.mark.parametrize("name", ["ultracomplex", "suzannes"])
def test_moved_scenes(name, helper):
    t = load_tris(name)[0]
    moved = HELPERS[helper](t)
    got = _assert_same(moved, f"{name} {helper}")
    if helper == "scatter":  # (the point of a regroup: the moved geometry groups otherwise)
        assert not np.array_equal(got, upload_membership(t))


@pytest.mark.parametrize("n", COUNTS)
def test_synthetic_sizes(n):
    t = synthetic(n)
    got = _assert_same(t, f"n{n}")
    assert np.array_equal(got, median_split(centroids(t)))


def test_empty_scene():
    assert rt.regroup_membership_host(np.zeros(0, TRIANGLE_DT)).shape == (0,)
    assert rt.lib().rtc_regroup_membership_host(None, 0, None) == 0
    assert rt.lib().rtc_regroup_membership_host(None, -1, None) == RTC_EINVAL
    assert rt.lib().rtc_regroup_membership_host(None, 3, None) == RTC_EINVAL


# ---- designed inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 40, 257])
def test_equal_centroids_give_the_identity(n):
    t = at(np.tile([[0.5, -1.0, 3.0]], (n, 1)))
    got = _assert_same(t, f"{n} equal centroids")
    assert np.array_equal(got, np.arange(n)), "a stable sort of equal keys moves nothing"


def test_ties_keep_their_position_not_their_index():
    """Level 0 sorts along x and reverses the indices; level 1 sorts each half along y, whose keys come in groups of four
    equal ones: a stable sort keeps each group in the order of its positions after level 0 -- descending index -- where a
    tie broken by reference index would give ascending."""
    n = 32
    i = np.arange(n)
    t = at(np.stack([-1.0 * i, 6.0 * (i // 2 % 4), np.zeros(n)], 1))
    got = _assert_same(t, "ties")
    assert np.array_equal(got, median_split(centroids(t)))
    cent = centroids(t)
    for lo in (0, 16):
        half = got[lo:lo + 16]
        assert set(half.tolist()) == set(range(16, 32) if lo == 0 else range(16)), "level 0 sorts along x"
        y = cent[half, 1]
        assert (np.diff(y) >= 0).all(), "level 1 sorts each half along y"
        for v in np.unique(y):
            grp = half[y == v]
            assert len(grp) == 4 and (np.diff(grp) < 0).all(), f"ties at y = {v} must keep level 0's order: {grp}"


@pytest.mark.parametrize("axes, winner", [((0, 1), 0), ((1, 2), 1), ((0, 2), 0), ((0, 1, 2), 0)])
def test_equal_extents_take_the_lower_axis(axes, winner):
    """The centroids span exactly 15 along each axis of `axes` (and 0.5 along the others), in different orders per axis: the
    first split sorts along the lowest of them (a later axis must be strictly longer to win)."""
    n = 16
    i = np.arange(n)
    orders = {0: i, 1: (i * 5) % n, 2: (i * 7) % n}  # three different permutations of 0..15
    p = np.zeros((n, 3))
    for a in range(3):
        p[:, a] = orders[a] * (1.0 if a in axes else 1.0 / 32)
    t = at(p)
    got = _assert_same(t, f"equal extents {axes}")
    assert np.array_equal(got, median_split(centroids(t)))
    assert set(got[:8].tolist()) == set(np.flatnonzero(orders[winner] < 8).tolist())


def _poisoned(n, which, value, coords=("x",), verts=("posA", "posB", "posC")):
    t = synthetic(n)
    for v in verts:
        for c in coords:
            t[v][c][which] = value
    return t


@pytest.mark.parametrize("n", [40, 264])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 0.0, -0.0])
@pytest.mark.parametrize("every", [False, True])
def test_non_finite_and_zero_coordinates(n, value, every):
    """NaN, +inf, -inf, +0 and -0 vertex coordinates, in every fifth triangle or in all of them, along one axis and along
    all three; and infinities in one vertex alone (AB = inf - x: an infinite or NaN centroid)."""
    which = slice(None) if every else slice(1, None, 5)
    for coords in (("x",), ("x", "y", "z")):
        t = _poisoned(n, which, value, coords)
        _assert_same(t, f"n{n} {value} {coords} every={every}")
    t = _poisoned(n, which, value, ("y",), verts=("posB",))
    _assert_same(t, f"n{n} {value} in posB alone")


def test_mixed_poison():
    """NaN, both infinities and both zeros together, and +0 / -0 keys side by side (they tie: position decides)."""
    n = 264
    t = synthetic(n)
    vals = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    for k, v in enumerate(vals):
        for vert in VERTS:
            t[vert]["x"][k::11] = v
    got = _assert_same(t, "mixed")
    assert np.array_equal(got, median_split(centroids(t)))
    z = at(np.stack([np.where(np.arange(40) % 2, 0.0, -0.0), np.zeros(40), np.zeros(40)], 1))
    for vert in VERTS:  # (exact signed zeros: no edge offsets along x)
        z[vert]["x"] = np.where(np.arange(40) % 2, 0.0, -0.0).astype(np.float32)
    assert np.array_equal(_assert_same(z, "signed zeros"), np.arange(40))


# ---- the interface and the refusals that need no device -----------------------------------------------------------------
def test_symbols_and_python_surface():
    L = rt.lib()
    names = {"rtc_scene_regroup_scratch_bytes", "rtc_scene_regroup_max_tris", "rtc_scene_regroup_async", "rtc_scene_regroup",
             "rtc_regroup_membership_host", "rtc_plan_sim_regroup"}
    assert all(hasattr(L, n) for n in names) and names <= set(_abi.EXPORTS)
    for f in ("regroup_membership_host", "regroup_max_tris"):
        assert callable(getattr(rt, f)) and f in rt.__all__
    for m in ("regroup_async", "regroup_scratch_bytes", "update"):
        assert hasattr(rt.DeviceScene, m)
    import inspect

    p = inspect.signature(rt.DeviceScene.update).parameters
    assert list(p)[1:] == ["tris", "spheres", "stream", "regroup"] and p["regroup"].default is False


def test_null_scene_is_refused_before_any_device_call():
    L = rt.lib()
    t = synthetic(9)
    p = t.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(0x7F0000001000)  # (never read: the scene is checked first)
    assert L.rtc_scene_regroup_async(None, fake, 9, None, 0, fake, 1 << 20, None) == RTC_EINVAL
    assert b"rtc_scene_regroup_async" in L.rtc_last_error() and b"null scene" in L.rtc_last_error()
    assert L.rtc_scene_regroup(None, p, 9, None, 0) == RTC_EINVAL
    assert b"rtc_scene_regroup" in L.rtc_last_error() and b"null scene" in L.rtc_last_error()
    assert L.rtc_scene_regroup_scratch_bytes(None) == 0


def test_max_tris():
    """A power of two that covers the project's scenes; the same on every call; the planner's hook refuses a scene above it
    and takes one at it."""
    cap = rt.regroup_max_tris()
    assert cap == rt.regroup_max_tris() == rt.lib().rtc_scene_regroup_max_tris()
    assert cap >= 4096 and cap & (cap - 1) == 0
    L = rt.lib()
    ops, fp = (C.c_int * 1024)(), (C.c_ulonglong * (6 * 256))()
    for n, ok in ((cap, True), (cap + 1, False), (cap - 7, True)):
        h = C.c_void_p()
        assert L.rtc_plan_sim_create(n, 0, C.byref(h)) == 0
        try:
            rc = L.rtc_plan_sim_regroup(h, 0, 0x5000, ops, 256, fp, 256)
            assert (rc > 0) == ok and (ok or rc == RTC_EINVAL), (n, rc)
        finally:
            L.rtc_plan_sim_release(h)
