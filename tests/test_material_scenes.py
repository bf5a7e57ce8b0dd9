"""The material scenes (tests/material_scenes.py) are not vacuous: every claim a note makes is shown here without the code
under test -- with the CPU oracle's recorded paths (oracle.calc_path: per calculateRayCollision call the ray, the winner,
dst, the roulette's p and draw), numpy restatements of the kernel's gates and the library's host statements of what an
upload builds (scene_records_host, bounce_hit_share: host code, no GPU).  tests/test_gpu_materials.py renders the frames.  A
scene that misses a claim is changed, not the claim.

State indices and windows as in tests/test_chain_path_scenes.py: S_j is the sample started from the pixel's seed advanced by
7 j draws; lane l of the window at jn evaluates S_{jn + l} and is alive at iteration i exactly when S_{jn + l} makes more
than i calls (iteration 0 is the primary ray).  rho = |dir|_1 is formed in float32 as the kernel forms it."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import progressive_reference as pr
import raytracingc_amd as rt
from chain_path_scenes import CHUNK_CLUSTERS, CLUSTER, DENSE_CULL_MAX, PASS_SPLIT, WGS_HIT_SHARE, clusters_of
from material_scenes import (EDGES, EVERY, NONFINITE_EVERY, FRAMES, GEOMETRIES, LADDER, NAN_FRAMES, ORDINARY, PASS_FRAMES, SCENES,
                             SPHERE_FRAME, SPHERE_NAMES, sky, sphere_scene)
from primary_rays import launch_rays
from test_chain_path_scenes import walk

F = np.float32
RHO_MAX = F(4.0)  # rtc_layout.h kClusterRhoMax
WINDOW_PIXELS = (0, 5, 100, 137, 250, 333, 402, 479)  # of the ladder's 24 x 20 frames


def _cfg(W, H, spp, mb):
    return rt.RenderConfig(W, H, spp, mb, True)


def rho_of(d):
    """|dir|_1 as chain_trace_pairs forms it: fabsf(x) + fabsf(y) + fabsf(z), float32, left to right."""
    with np.errstate(all="ignore"):
        a = np.abs(d.astype(F))
        return ((a[..., 0] + a[..., 1]).astype(F) + a[..., 2]).astype(F)


@functools.lru_cache(maxsize=None)
def state_paths(scene_name, W, H, mb, pixels, n):
    """calc_path of S_0 .. S_{n-1} of the pixels `pixels` (launch indices): (calls CALL_DT [pixels, n, mb], ncalls
    [pixels, n])."""
    tris = SCENES[scene_name][0]
    cam = SCENES[scene_name][1]
    cfg = _cfg(W, H, 1, mb)
    d = cfg.desc()
    px = np.array(pixels)
    rays = launch_rays(cam, cfg)[px]
    s = pr.seeds(d)[px]
    states = []
    for _ in range(n):
        states.append(s)
        s = pr.advance(s, 7)
    _, _, calls, ncalls = orc.calc_path(tris, None, rt.default_scene(), 1, np.tile(rays, n), np.concatenate(states),
                                        np.full(n * len(px), mb, np.int32))
    calls = calls.reshape(n, len(px), -1).transpose(1, 0, 2).copy()
    ncalls = ncalls.reshape(n, len(px)).T.copy()
    calls.setflags(write=False)
    ncalls.setflags(write=False)
    return calls, ncalls


@functools.lru_cache(maxsize=None)
def frame_paths(frame):
    """The frame's own samples in order, every pixel: (calls CALL_DT [spp, pixels, mb], ncalls [spp, pixels], radiance
    float32 [spp, pixels, 3]); each sample checked against calc_color (colour bits and seed)."""
    scene_name, W, H, spp, mb = FRAMES[frame]
    tris, cam, _ = SCENES[scene_name]
    cfg = _cfg(W, H, spp, mb)
    d = cfg.desc()
    rays, s = launch_rays(cam, cfg), pr.seeds(d)
    mbs = np.full(len(rays), mb, np.int32)
    out, nout, rad = [], [], []
    for _ in range(spp):
        col, after, calls, ncalls = orc.calc_path(tris, None, sky(frame), 1, rays, s, mbs)
        col2, after2 = orc.calc_color(tris, None, sky(frame), 1, rays, s, mbs)
        nan = np.isnan(col2)
        assert np.array_equal(np.isnan(col), nan) and np.array_equal(col.view(np.uint32)[~nan], col2.view(np.uint32)[~nan])
        assert np.array_equal(after, after2)
        out.append(calls)
        nout.append(ncalls)
        rad.append(col)
        s = after
    res = np.stack(out), np.stack(nout), np.stack(rad)
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def oracle_frame(frame, which="own"):
    """The oracle's (u8, floats, segments) of the frame; which = "ordinary": with ORDINARY's materials, "sky": no triangles."""
    scene_name, W, H, spp, mb = FRAMES[frame]
    tris, cam, _ = SCENES[scene_name]
    tris = {"own": tris, "ordinary": ORDINARY[scene_name], "sky": tris[:0]}[which]
    col, acc, seg = orc.render(tris, None, sky(frame), cam, _cfg(W, H, spp, mb).desc(), threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


def hits_of(calls, ncalls):
    """Hits per path: its calls, less the last one where that is a miss."""
    last = np.take_along_axis(calls["winner"], np.maximum(ncalls - 1, 0)[..., None], -1)[..., 0]
    return ncalls - ((ncalls > 0) & (last == -1))


def windows(scene_name, W, H, spp, mb):
    """Per pixel of WINDOW_PIXELS the windows of rtc_render_chain, each as (nAct, ncalls of its lanes, calls of its lanes)."""
    n = spp * mb + 64 + mb
    calls, ncalls = state_paths(scene_name, W, H, mb, WINDOW_PIXELS, n)
    out = []
    for p in range(len(WINDOW_PIXELS)):
        h = hits_of(calls[p], ncalls[p])
        for jn, n_act, _ in walk(lambda j: int(h[j]), spp):
            out.append((n_act, ncalls[p, jn:jn + n_act], calls[p, jn:jn + n_act]))
    return out


def lanes_at(window, i):
    """(rho of the lanes alive at iteration i, beyond = rho > 4; NaN counts as beyond: rho <= 4 is what the gate asks)."""
    _, nc, calls = window
    alive = nc > i
    rho = rho_of(calls["dir"][alive, i]) if i < calls.shape[1] else np.zeros(0, F)
    with np.errstate(invalid="ignore"):
        return rho, ~(rho <= RHO_MAX)


# ---- the table ------------------------------------------------------------------------------------------------------------
def test_scene_table_is_as_specified():
    for name, (tris, cam, note) in SCENES.items():
        assert name.split("_")[0] in note
        # windings equal stored normals: AB x AC along the normal (the reference recomputes it)
        g = lambda k: np.stack([tris[k][c] for c in "xyz"], 1).astype(np.float64)  # noqa: E731
        n = np.cross(g("posB") - g("posA"), g("posC") - g("posA"))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        assert np.allclose(n, g("normal"), atol=1e-6), name
        assert len(ORDINARY[name]) == len(tris)
    for g in GEOMETRIES:
        for tag, s in LADDER.items():
            t = SCENES[f"{g}_s{tag}"][0]
            assert (t["mat"]["smoothness"] == F(s)).all() and (t["mat"]["color"]["x"] == 1).all()
            m = np.stack([t["mat"]["color"]["y"], t["mat"]["color"]["z"], t["mat"]["emissionStrength"]], 1)
            assert len(np.unique(m, axis=0)) == len(t), "two triangles share a material"
    assert clusters_of(len(SCENES["shell_s2"][0])) == 3 and clusters_of(len(SCENES["boxT_s2"][0])) == 18
    assert clusters_of(len(SCENES["fine_s2"][0])) >= CHUNK_CLUSTERS + 1
    assert set(LADDER.values()) == {-1.0, 2.0, 2.5, 8.0, 1e6, 3e38}
    for name, (scene, W, H, spp, mb) in FRAMES.items():
        assert W <= 48 and H <= 40 and spp <= 64 and scene in SCENES and (mb <= 10 or (W, H, spp, mb) == (16, 8, 5, 65))
    assert FRAMES["shell_s2p5_mb65"] == ("shell_s2p5", 16, 8, 5, 65)
    for kind, where in ((k, w) for k in EDGES for w in ("cbox", "copen")):
        t, o = SCENES[f"{where}_{kind}"][0], ORDINARY[f"{where}_{kind}"]
        same = np.array([t[i]["mat"].tobytes() == o[i]["mat"].tobytes() for i in range(len(t))])
        i = np.arange(len(t))
        # nonfinite: each material once or twice; bright and negative materials on 2, 6, 10, ..
        extreme = (i % NONFINITE_EVERY[where] == 0) | (i % 4 == 2) if kind == "nonfinite" else i % EVERY == 0
        assert not same[extreme].any() and same[~extreme].all()
        assert kind != "nonfinite" or extreme[::NONFINITE_EVERY[where]].sum() >= len(EDGES[kind])
    for f, (scene, W, H, mb) in PASS_FRAMES.items():
        assert FRAMES[f] == (scene, W, H, sum(PASS_SPLIT), mb)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_hit_share_is_on_the_side_the_note_says(name):
    tris, _, note = SCENES[name]
    share = rt.bounce_hit_share(tris)
    print(f"{name}: bounce_hit_share {share:.4f}")
    if "not hit-heavy" in note:
        assert share < WGS_HIT_SHARE
    else:
        assert "hit-heavy" in note and share > WGS_HIT_SHARE


# ---- calc_path is calc_color ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_recorded_paths_are_calc_colors(frame):
    """calc_path's colour and seed equal calc_color's on every sample of the frame (asserted in frame_paths), the samples
    summed as main.c:99 sums them are oracle.render's accumulator, and the calls recorded are oracle.render's segments."""
    scene_name, W, H, spp, mb = FRAMES[frame]
    calls, ncalls, rad = frame_paths(frame)
    _, oacc, oseg = oracle_frame(frame)
    w = F(1.0 / np.float64(spp))
    acc = np.zeros(rad.shape[1:], F)
    with np.errstate(all="ignore"):
        for k in range(spp):
            acc = (acc + (rad[k] * w).astype(F)).astype(F)
    nan = np.isnan(oacc.reshape(-1, 3))
    assert np.array_equal(np.isnan(acc), nan)
    assert np.array_equal(acc.view(np.uint32)[~nan], oacc.reshape(-1, 3).view(np.uint32)[~nan])
    assert int(ncalls.sum()) == oseg


# ---- the smoothness ladder ------------------------------------------------------------------------------------------------
def _ladder_windows(g, tag):
    scene_name, W, H, spp, mb = FRAMES[f"{g}_s{tag}"]
    return windows(scene_name, W, H, spp, mb)


@pytest.mark.parametrize("g", sorted(GEOMETRIES))
def test_s2_drops_the_table_for_a_few_lanes(g):
    """smoothness 2: a full window whose first bounce has 1..4 lanes beyond rho = 4 and at least 32 within (the ballot
    drops the table for all of them) and another with none beyond (the table mode runs)."""
    full = [w for w in _ladder_windows(g, "2") if w[0] == 64]
    assert len(full) >= 8
    beyond = [int(lanes_at(w, 1)[1].sum()) for w in full]
    within = [int((~lanes_at(w, 1)[1]).sum()) for w in full]
    print(f"{g}_s2: full windows {len(full)}; lanes beyond 4 at iteration 1, by count: {np.bincount(beyond).tolist()}")
    assert any(1 <= b <= 4 and i >= 32 for b, i in zip(beyond, within))
    assert any(b == 0 and i >= 32 for b, i in zip(beyond, within))


@pytest.mark.parametrize("g", sorted(GEOMETRIES))
def test_s2p5_mixes_every_cull(g):
    """smoothness 2.5: at least half the full windows have >= 8 lanes on each side of rho = 4 at the first bounce; at some
    iteration >= 2 a window holds live lanes on both sides, once with <= 16 live lanes (the dense cull) and once with more
    (the per-lane loop, fusedG, the chunk cull)."""
    scene_name, W, H, spp, mb = FRAMES[f"{g}_s2p5"]
    ws = _ladder_windows(g, "2p5")
    full = [w for w in ws if w[0] == 64]
    mixed = 0
    for w in full:
        _, b = lanes_at(w, 1)
        mixed += b.sum() >= 8 and (~b).sum() >= 8
    dense = loop = 0
    for w in ws:
        for i in range(2, mb):
            _, b = lanes_at(w, i)
            if b.any() and (~b).any():
                dense += len(b) <= DENSE_CULL_MAX
                loop += len(b) > DENSE_CULL_MAX
    print(f"{g}_s2p5: {mixed} of {len(full)} full windows mixed at iteration 1; (window, iteration >= 2) pairs with both "
          f"sides live: {dense} dense, {loop} above {DENSE_CULL_MAX} lanes")
    assert len(full) >= 8 and 2 * mixed >= len(full)
    assert loop >= 1
    if clusters_of(len(SCENES[scene_name][0])) <= CHUNK_CLUSTERS:  # (MULTI has no dense cull: every live lane count runs its loop)
        assert dense >= 1


@pytest.mark.parametrize("g", sorted(GEOMETRIES))
def test_s8_is_beyond_the_bound_from_the_first_bounce(g):
    ws = _ladder_windows(g, "8")
    b = np.concatenate([lanes_at(w, 1)[1] for w in ws])
    print(f"{g}_s8: {b.mean():.4f} of {len(b)} iteration-1 lanes beyond 4")
    assert len(b) >= 512 and b.mean() >= 0.9


@pytest.mark.parametrize("g", sorted(GEOMETRIES))
def test_s1e6_leaves_the_box(g):
    """smoothness 1e6: no call after the first bounce records a hit, and every sample that bounced ends in an environment
    evaluation with |dir|_1 > 1e5."""
    calls, ncalls, _ = frame_paths(f"{g}_s1e6")
    assert (calls["winner"][..., 0] >= 0).all() and (ncalls >= 2).all()  # closed: every primary ray hits, p = 1 goes on
    valid = np.arange(calls.shape[2])[None, None, :] < ncalls[..., None]
    assert not (valid[..., 2:] & (calls["winner"][..., 2:] >= 0)).any()
    last = np.take_along_axis(calls, (ncalls - 1)[..., None], -1)[..., 0]
    rho = rho_of(last["dir"])
    second_hits = int((calls["winner"][..., 1] >= 0).sum())
    print(f"{g}_s1e6: {ncalls.size} samples, {second_hits} hit at the first bounce; the environment's |dir|_1: min "
          f"{rho.min():.4g}, median {np.median(rho):.4g}")
    assert (last["winner"] == -1).all() and (rho > F(1e5)).all()


@pytest.mark.parametrize("g", sorted(GEOMETRIES))
def test_s3e38_makes_inf_directions_and_nan_samples(g):
    """smoothness 3e38: samples with an inf direction component, and samples that are NaN.  The NaN is the environment's
    (inf * 0 in the sun term, inf - inf in its dot product), not a direction's: lerp(diffuse, specular, 3e38) sums a finite
    product and an infinite one, never inf - inf, and a ray with an inf component records no hit (every dst is NaN or below
    EPSILON), so no reflect ever sees one.  NaN directions are the nonfinite scenes' (smoothness inf and NaN), below."""
    calls, ncalls, rad = frame_paths(f"{g}_s3e38")
    d = calls["dir"]
    valid = np.arange(d.shape[2])[None, None, :] < ncalls[..., None]
    inf = (np.isinf(d).any(-1) & valid).any(-1)
    nan_dir = (np.isnan(d).any(-1) & valid).any(-1)
    nan = np.isnan(rad).any(-1)
    print(f"{g}_s3e38: of {inf.size} samples {int(inf.sum())} have an inf direction component, {int(nan_dir.sum())} a NaN one, "
          f"{int(nan.sum())} are NaN")
    assert inf.sum() >= 1 and nan.sum() >= 1 and nan_dir.sum() == 0


@pytest.mark.parametrize("frame", ["cbox_nonfinite", "copen_nonfinite"])
def test_nonfinite_smoothness_makes_nan_directions(frame):
    calls, ncalls, _ = frame_paths(frame)
    d = calls["dir"]
    valid = np.arange(d.shape[2])[None, None, :] < ncalls[..., None]
    nan = int((np.isnan(d).any(-1) & valid).any(-1).sum())
    inf = int((np.isinf(d).any(-1) & valid).any(-1).sum())
    print(f"{frame}: samples with a NaN direction component {nan}, with an inf one {inf}")
    assert nan >= 10


# ---- the clusters ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cluster_of_triangle(scene_name):
    """(cluster of every triangle, balls float32 [clusters, 8]) from the library's host statement of the records."""
    tris = SCENES[scene_name][0]
    rec = rt.scene_records_host(tris)
    idx = rec["clTris"][:, 12].view(np.int32)
    cl = np.full(len(tris), -1)
    cl[idx[idx >= 0]] = np.flatnonzero(idx >= 0) // CLUSTER
    assert (cl >= 0).all()
    return cl, rec["clusters"].view(F).copy()


def ball_would_cull(pos, d, ball):
    """cluster_culled (rtc_layout.h) restated in double, WITHOUT the gate on rho: cluster_terms, then culled_by."""
    pos, d, ball = pos.astype(np.float64), d.astype(np.float64), ball.astype(np.float64)
    with np.errstate(all="ignore"):
        w = ball[:, 0:3] - pos
        S = np.abs(w).sum(-1) + ball[:, 3]
        w2 = (w * w).sum(-1)
        A = (ball[:, 3] + 2e-5 * S) + ball[:, 6]
        B = ball[:, 5] * S + ball[:, 4]
        rho = np.abs(d).sum(-1)
        T = (rho * B + A) * 1.00001
        dd = (d * d).sum(-1)
        b = (w * d).sum(-1)
        wd = w2 * dd
        return np.where(b > 0, (wd - b * b) - 1.5e-6 * wd > T * T * dd, w2 > T * T)


def hit_calls(frame):
    """The calls of the frame's samples that recorded a hit, flat."""
    calls, ncalls, _ = frame_paths(frame)
    valid = np.arange(calls.shape[2])[None, None, :] < ncalls[..., None]
    return calls[valid & (calls["winner"] != -1)]


def _gate_counts(frame):
    scene_name = FRAMES[frame][0]
    cl, balls = cluster_of_triangle(scene_name)
    c = hit_calls(frame)
    rho = rho_of(c["dir"])
    with np.errstate(invalid="ignore"):
        c = c[rho > RHO_MAX]
    k = cl[c["winner"]]
    would = ball_would_cull(c["pos"], c["dir"], balls[k])
    return len(c), int(would.sum()), c, k


@pytest.mark.parametrize("frame", ["boxT_s2p5", "boxT_s8", "fine_s2p5", "fine_s8", "shell_s2p5", "shell_s8"])
def test_hits_beyond_the_bound_and_what_the_ball_test_makes_of_them(frame):
    """The frame has thousands of hits by rays with rho > 4, which every cull must let through.  How many of them lie in a
    cluster that cluster_culled, evaluated regardless of rho, would cull -- the hits a kernel that ignored the gate would
    lose?  None, here and (by the following argument) in any finite scene, so no frame can tell such a kernel from the
    library's: the gate is the proof's premise, not a condition the arithmetic needs.  The threshold T = A + rho B has
    B >= beta S with beta = 4 k 45 u E^2 / EPSILON, so T > S -- farther than the half-line ever is from a ball whose centre
    is within S of its origin -- as soon as 0.0107 E^2 rho > 1; below that 8 u E^2 rho / EPSILON < 0.045, where the error
    bound the threshold is built from holds with k = 1.05, inside the safety factor 4.  Measured: 0 of 183,703 (boxT, 2.5),
    0 of 69,235 (boxT, 8), 0 of 109,338 (fine, 2.5).  The test keeps the count at zero: a change of the constants that
    makes the gate matter shows here first.  (What the gate does change is work, and
    tests/test_gpu_materials.py::test_rays_beyond_the_bound_visit_every_triangle holds the kernels to it by their counters.)"""
    n, would, _, _ = _gate_counts(frame)
    print(f"{frame}: {n} hits by rays with rho > 4, {would} of them in a cluster the ball test alone would cull")
    assert n >= 1000 and would == 0


@pytest.mark.parametrize("tag", ["2p5", "8"])
def test_multi_scene_hits_past_the_first_chunk_beyond_the_bound(tag):
    """fine (MULTI): lanes with rho > 4 whose ray hits a triangle outside the first chunk (cluster >= 32)."""
    n, _, c, k = _gate_counts(f"fine_s{tag}")
    later = int((k >= CHUNK_CLUSTERS).sum())
    print(f"fine_s{tag}: {later} of {n} hits by rays with rho > 4 lie past the first chunk")
    assert later >= 1


def test_layers17_floor_mixes_the_first_bounce():
    """layers17_s2p5: first-bounce windows of floor pixels with lanes on both sides of rho = 4 (the separate cull and pair
    build runs for the lanes within, the wave's table is dropped where any lane is beyond)."""
    calls, ncalls, _ = frame_paths("layers17_s2p5")
    tris = SCENES["layers17_s2p5"][0]
    floor = calls["winner"][0, :, 0] >= len(tris) - 2
    assert floor.sum() >= 100
    rho = rho_of(calls["dir"][:, floor, 1])
    assert (ncalls[:, floor] >= 2).all()
    share = float((rho > RHO_MAX).mean())
    print(f"layers17_s2p5: {int(floor.sum())} floor pixels; {share:.3f} of their first bounces beyond 4")
    assert 0.1 < share < 0.9


# ---- colours and emission -----------------------------------------------------------------------------------------------
def _p_counts(frame):
    c = hit_calls(frame)
    p, rc = c["p"], c["rayColor"]
    with np.errstate(invalid="ignore"):
        return {"+0": int(((p == 0) & ~np.signbit(p)).sum()), "-0": int(((p == 0) & np.signbit(p)).sum()),
                ">1": int((p > 1).sum()), "<0": int((p < 0).sum()),
                "finite_with_nan": int((np.isfinite(p) & np.isnan(rc).any(-1)).sum()), "nan": int(np.isnan(p).sum()),
                "inf": int(np.isposinf(p).sum())}


def _acc_counts(frame):
    acc = oracle_frame(frame)[1]
    px = lambda m: int(m.any(-1).sum())  # noqa: E731
    with np.errstate(invalid="ignore"):
        return {"+inf": px(np.isposinf(acc)), "-inf": px(np.isneginf(acc)), "nan": px(np.isnan(acc)), "negative": px(acc < 0),
                "finite>=1": px(np.isfinite(acc) & (acc >= 1))}


COLOUR_CLAIMS = {"zero": (("+0", "-0"), ()), "bright": ((">1",), ("finite>=1",)), "negative": (("<0",), ("negative",)),
                 "blinding": ((">1",), ("+inf", "nan")), "nonfinite": (("finite_with_nan", "nan", "inf"), ("nan",))}
# in the open scene alone: a pixel all of whose infinite samples are negative (in the closed box every pixel with a -inf
# sample has a +inf one too, and is NaN), and paths that pass two negative colours
OPEN_CLAIMS = {"blinding": ((), ("-inf",)), "nonfinite": ((), ("negative",))}
BOX_CLAIMS = {"nonfinite": (("<0", "-0"), ())}


@pytest.mark.parametrize("where", ["cbox", "copen"])
@pytest.mark.parametrize("kind", sorted(EDGES))
def test_colour_frames_reach_their_values(kind, where):
    frame = f"{where}_{kind}"
    p, a = _p_counts(frame), _acc_counts(frame)
    print(f"{frame}: samples by p {p}; pixels by accumulator {a}")
    extra = (OPEN_CLAIMS if where == "copen" else BOX_CLAIMS).get(kind, ((), ()))
    for k in COLOUR_CLAIMS[kind][0] + extra[0]:
        assert p[k] >= 10, f"{frame}: p {k}"
    for k in COLOUR_CLAIMS[kind][1] + extra[1]:
        assert a[k] >= 10, f"{frame}: accumulator {k}"


@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_nan_cap(frame):
    """NaN positions are left out of the bit comparison, so they are capped: no NaN at all outside the blinding, nonfinite
    and 3e38 frames, at most half the accumulator there, and at least a quarter of the pixels with a value that is not NaN
    and differs from the same geometry's frame with ordinary materials."""
    scene_name, W, H, spp, mb = FRAMES[frame]
    acc, plain, empty = oracle_frame(frame)[1], oracle_frame(frame, "ordinary")[1], oracle_frame(frame, "sky")[1]
    geometry = (plain.view(np.uint32) != empty.view(np.uint32)).any(-1)
    nan = np.isnan(acc)
    differs = (~nan & (acc.view(np.uint32) != plain.view(np.uint32))).any(-1) & geometry
    print(f"{frame}: NaN share {nan.mean():.4f}; {int(differs.sum())} of {int(geometry.sum())} geometry pixels differ from "
          f"the ordinary materials' frame in a value that is not NaN")
    assert not np.isnan(plain).any()
    if frame in NAN_FRAMES:
        assert nan.mean() <= 0.5
    else:
        assert not nan.any()
    assert geometry.sum() >= 100 and differs.sum() >= 0.25 * geometry.sum()


# ---- spheres ----------------------------------------------------------------------------------------------------------------
def open5_like(sph):
    """The same spheres with sphere_scenes.open5's ordinary materials."""
    from sphere_scenes import open5

    o = sph.copy()
    o["mat"][:5] = open5()["mat"]
    return o


@pytest.mark.parametrize("name", SPHERE_NAMES)
def test_sphere_scenes_probe_and_reach(name):
    """bounce_hit_share (host code) is finite and in [0, 1] on the sphere scenes; the routing the GPU tests expect follows
    from it (at most 0.5: the split launch).  Every one of the five spheres wins hits -- the zero behind the camera by bounce
    rays only --, rays leave the smoothness-2.5 and -8 spheres with rho > 4, the blinding lamp makes pixels inf and NaN, and
    the NaN positions, left out of the bit comparison, are capped as in test_nan_cap.  calc_path's colour and seed are
    calc_color's on every sample, and the samples summed are oracle.render's frame."""
    tris, sph, cam, _ = sphere_scene(name)
    share = rt.bounce_hit_share(tris, sph)
    print(f"{name}: bounce_hit_share {share:.4f}")
    assert np.isfinite(share) and 0.0 <= share <= 1.0
    assert (share <= 0.5) == (name != "spheres_closed")
    W, H, spp, mb = SPHERE_FRAME
    cfg = rt.RenderConfig(W, H, spp, mb, False)
    d = cfg.desc()
    rays, s = launch_rays(cam, cfg), pr.seeds(d)
    mbs = np.full(len(rays), mb, np.int32)
    winners, beyond, primary, segments = np.zeros(len(sph), np.int64), 0, np.zeros(len(sph), np.int64), 0
    sums, w32 = np.zeros((len(rays), 3), F), F(1.0 / np.float64(spp))
    for _ in range(spp):
        col, after, calls, ncalls = orc.calc_path(tris, sph, rt.default_scene(), 0, rays, s, mbs)
        col2, after2 = orc.calc_color(tris, sph, rt.default_scene(), 0, rays, s, mbs)
        nan = np.isnan(col2)
        assert np.array_equal(np.isnan(col), nan) and np.array_equal(col.view(np.uint32)[~nan], col2.view(np.uint32)[~nan])
        assert np.array_equal(after, after2)
        s = after
        with np.errstate(all="ignore"):
            sums = (sums + (col * w32).astype(F)).astype(F)
        segments += int(ncalls.sum())
        valid = np.arange(calls.shape[1])[None, :] < ncalls[:, None]
        w = calls["winner"][valid]
        winners += np.bincount(-2 - w[w <= -2], minlength=len(sph))
        w0 = calls["winner"][:, 0]
        primary += np.bincount(-2 - w0[w0 <= -2], minlength=len(sph))
        prev = np.zeros(valid.shape, bool)
        prev[:, 1:] = (calls["winner"][:, :-1] <= -2) & (calls["winner"][:, :-1] >= -3) & valid[:, 1:]
        with np.errstate(invalid="ignore"):
            beyond += int((rho_of(calls["dir"][prev]) > RHO_MAX).sum())
    print(f"{name}: hits won per sphere {winners.tolist()} (at the primary hit {primary.tolist()}); rays leaving spheres 0 "
          f"and 1 with rho > 4: {beyond}")
    assert (winners[:5] >= 10).all() and beyond >= 10
    assert primary[2] >= 10 and primary[3] >= 10  # (the blinding lamp and the ground are loaded at the primary hit too)
    _, acc, seg = orc.render(tris, sph, rt.default_scene(), cam, d, threads=16)
    plain = orc.render(tris, open5_like(sph), rt.default_scene(), cam, d, threads=16)[1]
    empty = orc.render(tris[:0], None, rt.default_scene(), cam, rt.RenderConfig(W, H, spp, mb, True).desc(), threads=16)[1]
    nan = np.isnan(acc)
    assert np.array_equal(np.isnan(sums), nan.reshape(-1, 3)) and seg == segments
    assert np.array_equal(sums.view(np.uint32)[~nan.reshape(-1, 3)], acc.reshape(-1, 3).view(np.uint32)[~nan.reshape(-1, 3)])
    geometry = (plain.view(np.uint32) != empty.view(np.uint32)).any(-1)
    differs = (~nan & (acc.view(np.uint32) != plain.view(np.uint32))).any(-1) & geometry
    px = lambda m: int(m.any(-1).sum())  # noqa: E731
    print(f"{name}: pixels +inf {px(np.isposinf(acc))}, -inf {px(np.isneginf(acc))}, NaN {px(nan)}; NaN share "
          f"{nan.mean():.4f}; {int(differs.sum())} of {int(geometry.sum())} geometry pixels differ from the ordinary "
          f"materials' frame in a value that is not NaN")
    assert not np.isnan(plain).any()
    assert px(np.isinf(acc)) >= 10 and px(nan) >= 10 and nan.mean() <= 0.5
    assert geometry.sum() >= 100 and differs.sum() >= 0.25 * geometry.sum()


# ---- the roulette at equal zeros ------------------------------------------------------------------------------------------
def test_equal_zeros_follow_the_second_operand():
    """p = fmax(fmax(r, g), b) over zeros of mixed sign: the oracle's libm returns its second operand for equal values (the
    rule the device's fmax_ref states), so p carries the sign of the blue component -- all four sign patterns of the zero
    scene, each met by at least 10 hits.  No frame shows that sign: p = +0 or -0 is below every draw but 0."""
    c = hit_calls("cbox_zero")
    c = c[c["p"] == 0]
    rc = c["rayColor"]
    assert (rc == 0).all()
    seen = {}
    for pattern in ((False, False, False), (True, True, True), (True, False, True), (False, True, False)):
        m = (np.signbit(rc) == np.array(pattern)).all(-1)
        seen[pattern] = int(m.sum())
        assert m.sum() >= 10 and (np.signbit(c["p"][m]) == pattern[2]).all(), pattern
    print(f"cbox_zero: hits with p = 0 by the signs of rayColor: {seen}")


def test_a_draw_of_zero_goes_on_past_p_zero():
    """The one draw that p = +-0 is not below: RandomValue returns 0 exactly when the state after its step is 0.  From the seed
    that brings the roulette's draw -- the seventh of a hit -- to that state, a path whose first hit has a zero colour does
    not end there (-0 < 0 and +0 < 0 are false), divides by p and is NaN from then on, whatever the sign of p: even here
    the equal-zeros rule changes no colour."""
    a, inc = 747796405, 2891336453
    a_inv = pow(a, -1, 1 << 32)
    back = lambda s: ((s - inc) * a_inv) % (1 << 32)  # noqa: E731
    seed = 0
    for _ in range(7):  # the state whose seventh step gives 0
        seed = back(seed)
    u, _, _ = orc.random_sequences(np.array([seed], np.uint32), 7)
    assert u[0, 6] == 0 and (u[0, :6] > 0).all()
    scene_name, W, H, spp, mb = FRAMES["cbox_zero"]
    tris, cam, _ = SCENES[scene_name]
    calls, ncalls, _ = frame_paths("cbox_zero")
    first = calls[0, :, 0]
    px = np.flatnonzero((first["p"] == 0) & (first["winner"] >= 0))
    assert len(px) >= 10
    rays = launch_rays(cam, _cfg(W, H, 1, mb))[px]
    seeds, mbs = np.full(len(px), seed, np.uint32), np.full(len(px), 3, np.int32)
    col, after, got, n = orc.calc_path(tris, None, sky("cbox_zero"), 1, rays, seeds, mbs)
    col2, after2 = orc.calc_color(tris, None, sky("cbox_zero"), 1, rays, seeds, mbs)
    assert (got["draw"][:, 0] == 0).all() and (got["p"][:, 0] == 0).all() and (n >= 2).all()
    assert np.signbit(got["p"][:, 0]).any() and (~np.signbit(got["p"][:, 0])).any()
    assert np.isnan(col).all() and np.isnan(col2).all() and np.array_equal(after, after2)
