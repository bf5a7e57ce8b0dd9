"""The host statement of the scene records and of their refit (rtc_scene_records_host; rtc_scene.hip ball_of,
aligned_normal, rtc_cluster_records), without a GPU.  rtc_scene_update_async keeps the upload's cluster membership and
recomputes every record for the moved triangles; the device kernel is compared with this host statement byte for byte
(tests/test_gpu_scene_update.py), so here the statement itself is checked: an identity refit is the upload's build; after
a move every ball still holds every vertex of its records (the one property the culling proofs need), the
membership is the upload's, the aligned-normal flags and the never-cull escapes are those of independent numpy
restatements.  No reference counterpart (main.c:229-243 builds flat arrays once)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import raytracingc_amd as rt
from adversarial_scenes import SCENES as ADVERSARIAL
from conftest import load_tris
from moving_scenes import HELPERS, synthetic

U = 2.0 ** -24
RHO_MAX, EPS, GAMMA = 4.0, 0.001, float(np.float32(2e-5))
CLUSTER, CHUNK = 8, 32
SYNTHETIC = (1, 7, 8, 9, 255, 256, 257, 264)  # a partial last cluster, exactly one chunk, a second chunk of one cluster
NONFINITE = ("nonfinite", "mixed_scale", "bad_normals")  # NaN / inf vertices, 1e19 and 1e30 vertices, NaN normals
CASES = ["cube", "ultracomplex", "suzannes"] + [f"n{n}" for n in SYNTHETIC] + list(NONFINITE)


@functools.lru_cache(maxsize=None)
def triangles(case):
    if case in NONFINITE:
        t = ADVERSARIAL[case][0]
    elif case.startswith("n") and case[1:].isdigit():
        t = synthetic(int(case[1:]))
    else:
        t = load_tris(case)[0]
    t = t.copy()
    t.setflags(write=False)
    return t


def f32(rec):
    return rec.view(np.float32)


def vertices(cl_tris):
    """float64 [records, 3 vertices, 3]: A, A + AB, A + AC as ball_of forms them."""
    with np.errstate(all="ignore"):
        r = f32(cl_tris).astype(np.float64)
        a = r[:, 0:3]
        return np.stack([a, a + r[:, 3:6], a + r[:, 6:9]], 1)


def aligned_normal_numpy(cl_tris):
    """rtc_scene.hip aligned_normal, operation for operation in float64."""
    with np.errstate(all="ignore"):
        r = f32(cl_tris).astype(np.float64)
        AB, AC, N = r[:, 3:6].T, r[:, 6:9].T, r[:, 9:12].T
        G = [AB[1] * AC[2] - AB[2] * AC[1], AB[2] * AC[0] - AB[0] * AC[2], AB[0] * AC[1] - AB[1] * AC[0]]
        g = np.sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2])
        ok = (g > 0.0) & np.isfinite(g)
        a = (N[0] * G[0] + N[1] * G[1] + N[2] * G[2]) / g
        ok &= a > 0.0
        e = [N[k] - a * G[k] / g for k in range(3)]
        en = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + 1e-12 * (np.abs(N[0]) + np.abs(N[1]) + np.abs(N[2]))
        ninf = np.maximum(np.abs(N[0]), np.maximum(np.abs(N[1]), np.abs(N[2])))
        n1 = np.abs(AB[0]) + np.abs(AB[1]) + np.abs(AB[2])
        c1 = np.abs(AC[0]) + np.abs(AC[1]) + np.abs(AC[2])
        K = g * (3.01 * U * ninf + en) / a + 5.1 * U * n1 * c1
        return ok & np.isfinite(K) & (2.0 * RHO_MAX * K < 0.001)


def check_balls(cl_tris, balls, per_ball, what):
    """Every ball of `per_ball` consecutive records: it holds every vertex of its real records (float64, about the stored
    float centre and radius), and it carries the never-cull escape exactly when ball_of's conditions say so."""
    idx = cl_tris[:, 12].view(np.int32)
    v = vertices(cl_tris)
    b = f32(balls).astype(np.float64)
    with np.errstate(all="ignore"):
        edges = np.sqrt((f32(cl_tris).astype(np.float64)[:, 3:9].reshape(-1, 2, 3) ** 2).sum(-1)).max(-1)
    for k in range((len(cl_tris) + per_ball - 1) // per_ball):
        sl = slice(k * per_ball, min((k + 1) * per_ball, len(cl_tris)))
        real = idx[sl] >= 0
        vv = v[sl][real].reshape(-1, 3)
        c, r, alpha, beta, gamma_e = b[k, 0:3], b[k, 3], b[k, 4], b[k, 5], b[k, 6]
        finite = bool(np.isfinite(vv).all())
        with np.errstate(all="ignore"):
            E = float(np.nanmax(edges[sl][real], initial=0.0)) if real.any() else 0.0
            ed_ratio = 8.0 * U * E * E * RHO_MAX / EPS
        escape = (not finite) or (not real.any()) or not (ed_ratio < 0.5) or not (r < 1e18)
        if escape:
            assert np.isposinf(alpha) and beta == 0.0 and gamma_e == 0.0, f"{what}: ball {k} must never cull"
            continue
        assert np.isfinite([alpha, beta, gamma_e]).all() and alpha > 0 and beta > 0 and gamma_e >= GAMMA * E, \
            f"{what}: ball {k} margins"
        d = np.sqrt(((vv - c) ** 2).sum(-1))
        assert (d <= r).all(), f"{what}: ball {k} misses a vertex by {float((d - r).max())}"


@pytest.mark.parametrize("case", CASES)
def test_identity_refit_is_the_upload_build(case):
    t = triangles(case)
    a, b = rt.scene_records_host(t), rt.scene_records_host(t, t)
    for name in rt.RECORD_ARRAYS:
        assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), f"{case}: {name} differs"
    nc = (len(t) + CLUSTER - 1) // CLUSTER
    assert len(a["clTris"]) == max(nc * CLUSTER, 1) and len(a["clusters"]) == max(nc, 1)
    assert len(a["chunks"]) == max((nc + CHUNK - 1) // CHUNK, 1)


@pytest.mark.parametrize("helper", sorted(HELPERS))
@pytest.mark.parametrize("case", CASES)
def test_refit_records(case, helper):
    t = triangles(case)
    moved = HELPERS[helper](t)
    up, re = rt.scene_records_host(t), rt.scene_records_host(t, moved)
    what = f"{case} {helper}"
    # the membership is the upload's: the same permutation of the indices, padding in the same places
    pad0_up, pad0 = up["clTris"][:, 12].view(np.int32), re["clTris"][:, 12].view(np.int32)
    assert np.array_equal(pad0, pad0_up), f"{what}: membership changed"
    assert sorted(pad0[pad0 >= 0].tolist()) == list(range(len(t))), f"{what}: not a permutation"
    assert (pad0[len(t):] == -1).all()
    # the records in reference order are pack_scene's of the moved triangles; the clustered ones are those, reordered
    fresh = rt.scene_records_host(moved)
    assert np.array_equal(re["tris"], fresh["tris"]) and np.array_equal(re["mats"], fresh["mats"])
    real = pad0 >= 0
    assert np.array_equal(re["clTris"][real][:, :12], re["tris"][pad0[real]][:, :12])
    assert not re["clTris"][~real][:, :12].any() and not re["clTris"][:, 14:].any()
    # the aligned-normal flags
    flags = re["clTris"][:, 13].view(np.int32)
    want = aligned_normal_numpy(re["clTris"]) & real
    assert np.array_equal(flags, want.astype(np.int32)), f"{what}: {int((flags != want).sum())} aligned-normal flags"
    # the balls
    check_balls(re["clTris"], re["clusters"], CLUSTER, what + " clusters")
    check_balls(re["clTris"], re["chunks"], CLUSTER * CHUNK, what + " chunks")


@pytest.mark.parametrize("case", NONFINITE)
def test_nonfinite_vertices_never_cull(case):
    """The scenes with NaN / inf / 1e19+ vertices: the clusters and chunks that hold such a triangle carry alpha = +inf and
    beta = gamma E = 0 after a refit too (check_balls asserts it per ball; here: there is at least one such ball)."""
    t = triangles(case)
    re = rt.scene_records_host(t, HELPERS["shift"](t))
    check_balls(re["clTris"], re["clusters"], CLUSTER, case)
    if case != "bad_normals":  # (NaN normals touch no ball)
        assert np.isposinf(f32(re["clusters"])[:, 4]).any() and np.isposinf(f32(re["chunks"])[:, 4]).any()


def test_record_buffers_are_checked():
    """A buffer smaller than its array is refused (RTC_EINVAL), not overrun."""
    import ctypes as C

    t = np.ascontiguousarray(triangles("cube"))
    sizes = (C.c_size_t * 6)(*([16] * 6))
    small = np.zeros(4, np.uint32)
    rc = rt.lib().rtc_scene_records_host(t.ctypes.data_as(C.c_void_p), len(t), None, None, 0,
                                         small.ctypes.data_as(C.c_void_p), None, None, None, None, None, sizes)
    assert rc == rt.RTC_EINVAL
