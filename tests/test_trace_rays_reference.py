"""The premises of tests/test_gpu_trace_rays.py, from the CPU oracle alone (tests/trace_rays_reference.py), so that a GPU
test cannot pass on empty ground: the replay sets are the bounce rays the oracle's render traces and the expectation
reproduces their recorded winners and distances, they have hits and misses (and, for the default scene, sphere and
triangle winners), the scaled sets reach beyond the cluster bound's |dir|_1 <= 4 with hits and change winners at 1e-3 and
1e4, the primary set is the first-hit expectation, and the odd rays compute a NaN in one place only.  Reference:
calculateRayCollision (raytracing.c:216-240)."""
from __future__ import annotations

import numpy as np
import pytest

import first_hit_reference as fr
import trace_rays_reference as tr
from primary_rays import NO_HIT_DST


def _rho(rays):
    with np.errstate(all="ignore"):
        return np.abs(rays["dir"]["x"]) + np.abs(rays["dir"]["y"]) + np.abs(rays["dir"]["z"])


@pytest.mark.parametrize("name", sorted(tr.REPLAY))
def test_replay_sets(name):
    """The recorded calls after each pixel's first: as many rays and hits as measured when the sets were chosen, at least
    10 of each where both occur, and the expectation for those rays is the record's own winner and dst bit for bit."""
    calls, e = tr.replay_calls(name), tr.case_expected("replay", name)
    n_rays, n_hits = tr.REPLAY[name]
    hit = e["prim"] != -1
    print(f"{name}: {len(calls)} bounce rays, {int(hit.sum())} hits, {int((e['prim'] <= -2).sum())} on spheres")
    assert (len(calls), int(hit.sum())) == (n_rays, n_hits)
    assert np.array_equal(e["prim"], calls["winner"])
    assert np.array_equal(e["depth"].view(np.uint32), calls["dst"].astype(np.float32).view(np.uint32))
    assert hit.sum() >= 10 or n_hits < 10
    if n_rays - n_hits >= 10:
        assert (~hit).sum() >= 10
    assert (e["depth"][~hit] == NO_HIT_DST).all() and (e["depth"][hit] < NO_HIT_DST).all()
    assert not e["normal"][~hit].view(np.uint32).any() and not e["albedo"][~hit].view(np.uint32).any()
    if name == "default":
        assert int((e["prim"] <= -2).sum()) == tr.DEFAULT_SPHERE_HITS and (e["prim"] >= 0).sum() > 10
        assert len(tr.geometry(name)[1]) == 1 and tr.geometry(name)[2] == 0
    if name == "chunks":
        assert len(tr.geometry(name)[0]) == 288  # 36 clusters: more than one chunk
    assert not np.isnan(e["normal"]).any()


def test_replay_rays_start_on_the_geometry():
    """Bounce rays do not share an origin (what the kernel's per-lane ball tests are for)."""
    for name in ("chunks", "box_diffuse_T", "default"):
        r = tr.replay(name)
        assert len(np.unique(r["pos"])) > len(r) // 4


@pytest.mark.parametrize("name", tr.SCALED_CASES)
def test_scaled_sets(name):
    """x0.25 and x3 keep every hit (the EPSILON tests are far from these scales); x3 has hits with |dir|_1 > 4, where the
    kernel must not cull; x1e-3 and x1e4 change winners (the reference's EPSILON tests on det and dst see the scale)."""
    base = tr.case_expected("replay", name)
    for s in tr.SCALES:
        e, rays = tr.case_expected("scaled", name, s), tr.scaled(name, s)
        changed = int((e["prim"] != base["prim"]).sum())
        beyond = int(((_rho(rays) > tr.RHO_MAX) & (e["prim"] != -1)).sum())
        print(f"{name} x{s}: {int((e['prim'] != -1).sum())} hits, {changed} winners changed, {beyond} hits beyond rho 4")
        if s in (0.25, 3.0):
            assert (e["prim"] != -1).sum() == (base["prim"] != -1).sum()
        if s == 3.0:
            assert beyond >= 1 and float(_rho(rays).max()) > 5.0
        if s in (1e-3, 1e4) and name == "chunks":
            assert changed >= 10
            assert changed == {1e-3: 31, 1e4: 650}[s]
        assert not np.isnan(e["normal"]).any()


@pytest.mark.parametrize("name", sorted(n for n in tr.REPLAY if n != "default" and n not in tr.cps.SCENES))
def test_primary_set_is_the_first_hit_expectation(name):
    """(The cases first_hit_reference knows by the same name; the chain-path scenes' primary sets are launches' rays all
    the same, through the same two functions.)"""
    e, f = tr.case_expected("primary", name), fr.expected(name, tr.SHAPE)
    for k in tr.NAMES:
        assert np.array_equal(np.ascontiguousarray(e[k]).view(np.uint32).ravel(),
                              np.ascontiguousarray(f[k]).view(np.uint32).ravel()), k


def test_default_primary_set_is_the_first_hit_expectation():
    """The default scene with its sphere: first_hit_reference calls it default_spheres."""
    e, f = tr.case_expected("primary", "default"), fr.expected("default_spheres", tr.SHAPE)
    for k in tr.NAMES:
        assert np.array_equal(np.ascontiguousarray(e[k]).view(np.uint32).ravel(),
                              np.ascontiguousarray(f[k]).view(np.uint32).ravel()), k


def test_odd_rays():
    """With the sphere some odd rays hit it (a zero direction among them); NaN words occur only in `normal`, only on a
    sphere hit and in one ray: the zero direction from the sphere's centre.  With trianglesOnly nothing computed is NaN."""
    rays, labels = tr.odd()
    assert len(rays) == len(labels) >= 18
    e = tr.case_expected("odd", "default", None, 0)
    for l, p, d in zip(labels, e["prim"], e["depth"]):
        print(f"{l}: prim {p}, depth {d}")
    assert e["prim"][labels.index("dir = 0")] == -2 and e["prim"][labels.index("dir = 0 from the centre")] == -2
    assert (e["prim"] == -1).sum() >= 5 and (e["prim"] == -2).sum() >= 5
    nan_rows = np.isnan(e["normal"]).any(1)
    assert list(np.flatnonzero(nan_rows)) == [labels.index("dir = 0 from the centre")]
    assert (e["prim"][nan_rows] <= -2).all()
    assert not np.isnan(e["depth"]).any() and not np.isnan(e["albedo"]).any()
    t = tr.case_expected("odd", "default", None, 1)
    assert (t["prim"] >= -1).all() and (t["prim"] >= 0).any() and (t["prim"] == -1).any()
    assert not any(np.isnan(t[k]).any() for k in ("depth", "normal", "albedo"))


def test_extra_scenes():
    e = tr.case_expected("extra", "closing_sphere")
    assert (e["prim"] == -2).all() and tr.geometry("closing_sphere")[0] is None
    e = tr.case_expected("extra", "open33")
    assert len(e["prim"]) == tr.OPEN33_RAYS and (e["prim"] <= -2).any() and (e["prim"] >= 0).any()
    assert len(tr.geometry("open33")[1]) == 33
    for name in ("ties_axis", "ties_tilted", "ties_rotated"):
        assert (tr.case_expected("extra", name)["prim"] == 0).sum() > 50  # P0 wins the overlap with P1 (index 9)
    assert tr.case_expected("extra", "tie_scene")["prim"][tr.SHAPE[1] // 2 * tr.SHAPE[0] + tr.SHAPE[0] // 2] == -2
    for name in tr.EXTRA:
        tris = tr.geometry(name)[0]
        if name.startswith("counts_"):
            assert len(tris) == int(name.split("_")[1])
        if name.startswith("layers_"):
            assert len(tris) == 8 * int(name.split("_")[1])


def test_the_exception_for_nan_normals_is_narrow():
    """differing() lets a NaN differ in sign and payload only where the expected word is a NaN of a sphere hit."""
    want = {k: v.copy() for k, v in tr.case_expected("odd", "default", None, 0).items()}
    got = {k: v.copy() for k, v in want.items()}
    i = int(np.flatnonzero(np.isnan(want["normal"]).any(1))[0])
    got["normal"].view(np.uint32)[i] = 0xFFC00001
    assert tr.differing(got, want) == dict.fromkeys(tr.NAMES, 0)
    got["normal"][i] = 1.0
    assert tr.differing(got, want)["normal"] == 1
    got = {k: v.copy() for k, v in want.items()}
    j = int(np.flatnonzero(want["prim"] == -1)[0])
    got["normal"].view(np.uint32)[j, 0] = 0x7FC00000  # a NaN where +0 is expected
    assert tr.differing(got, want)["normal"] == 1
