"""The chain-path scenes (tests/chain_path_scenes.py) are not vacuous: every claim a note makes about the path its scene
takes is shown here without the code under test -- with the CPU oracle (oracle.ray_triangle, oracle.calc_color through
tests/progressive_reference.py), numpy float32 restatements of the kernel's switches, and the library's host statements of
what an upload builds (scene_records_host, bounce_hit_share: host code, no GPU).  tests/test_gpu_chain_paths.py renders the
frames; where a launch's own choice matters it reads it from DeviceScene.chain_report.  A scene that misses a claim is
changed, not the claim.

State indices (rtc_chain.h): S_j is the sample started from the pixel's seed advanced by 7 j draws; lane l of the window at
jn evaluates S_{jn + l} and is alive at bounce iteration i exactly when S_{jn + l} makes more than i calculateRayCollision
calls (iteration 0 is the primary ray)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import progressive_reference as pr
import raytracingc_amd as rt
from adversarial_scenes import ED_RATIO_EDGE
from chain_path_scenes import (CHAIN_PAIRS, CHUNK_CLUSTERS, CLUSTER, DENSE_CULL_MAX, FRAMES, LAYERS, MIRROR_BOUNCES,
                               PASS_FRAMES, PASS_SPLIT, SCENES, WGS_HIT_SHARE, clusters_of, first_unstaged, prim_f_staged)
from primary_rays import hit_table, launch_rays
from test_gpu_chain_paths import IN_KERNEL_SUMS, expected_report

F = np.float32


def _cfg(W, H, spp, mb):
    return rt.RenderConfig(W, H, spp, mb, True)


@functools.lru_cache(maxsize=None)
def state_samples(scene_name, W, H, mb, pixels, j0, n):
    """(hits, calls) int64 [len(pixels), n]: S_j0 .. S_{j0 + n - 1} of the frame's pixels `pixels` (launch indices)."""
    tris, cam, _ = SCENES[scene_name]
    cfg = _cfg(W, H, 1, mb)
    d = cfg.desc()
    px = np.array(pixels)
    rays = launch_rays(cam, cfg)[px]
    s = pr.advance(pr.seeds(d)[px], 7 * j0)
    states = []
    for _ in range(n):
        states.append(s)
        s = pr.advance(s, 7)
    _, _, calls, hits = pr.sample(tris, None, rt.default_scene(), d, np.tile(rays, n), np.concatenate(states))
    return hits.reshape(n, len(px)).T.copy(), calls.reshape(n, len(px)).T.copy()


def walk(hits_of, spp):
    """rtc_render_chain's windows restated from the hits per state index (hits_of(j)): per window (jn, nAct, samples
    committed).  est = ceil(need * jn / k) from the second window on, nAct = min(64, est + est / 8 + 1); the walk commits
    the sample at p and moves p on by its hits until p leaves the active lanes or the samples are done."""
    out, k, jn = [], 0, 0
    while k < spp:
        need = spp - k
        est = (need * jn + k - 1) // k if k > 0 else need
        n_act = min(64, est + (est >> 3) + 1)
        p, k0 = 0, k
        while k < spp and p < n_act:
            h = hits_of(jn + p)
            assert h >= 1
            k += 1
            p += h
        out.append((jn, n_act, k - k0))
        jn += p
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_scene_table_is_as_specified():
    for name, (tris, cam, note) in SCENES.items():
        m = np.stack([tris["mat"]["color"][c] for c in "xyz"] + [tris["mat"]["emissionStrength"], tris["mat"]["smoothness"]], 1)
        assert len(np.unique(m, axis=0)) == len(tris), f"{name}: two triangles share a material"
        assert name.split("_")[0] in note
    for n in LAYERS:
        assert clusters_of(len(SCENES[f"layers_{n}"][0])) == n and len(SCENES[f"layers_{n}"][0]) == 8 * n
    assert 16 * 64 <= CHAIN_PAIRS < 17 * 64 and CHUNK_CLUSTERS == 32
    assert clusters_of(len(SCENES["box_diffuse_T"][0])) == 18
    for name, (scene, W, H, spp, mb) in FRAMES.items():
        assert W <= 48 and H <= 40 and scene in SCENES
        if scene in ("box_mirror", "box_gloss"):
            assert W <= 16 and H <= 8
    assert {FRAMES[f"box_mirror_mb{m}"][4] for m in MIRROR_BOUNCES} == {63, 64, 65, 100}
    assert FRAMES["box_diffuse_deep"][3:] == (130, 40) and sum(PASS_SPLIT) == 64 and PASS_SPLIT[0] % 64 != 0


def test_prim_f_threshold_counts():
    """The derivation in chain_path_scenes: at 4 workgroups per CU the first unstaged single-chunk scene has 161 triangles
    (box_primf_4; box_primf_4_below is the 160 below); at 3 no single-chunk scene is unstaged -- 32 clusters still fit."""
    assert first_unstaged(4) == 161 == len(SCENES["box_primf_4"][0])
    assert len(SCENES["box_primf_4_below"][0]) == 160 and prim_f_staged(160, 4) and not prim_f_staged(161, 4)
    assert first_unstaged(3) is None and prim_f_staged(256, 3) and prim_f_staged(161, 3)
    assert not prim_f_staged(257, 3)  # (two chunks: MULTI never stages)
    # box_diffuse_T runs the kernel without the GENERAL code at 4 workgroups per CU only while staged: 17..20 clusters
    assert prim_f_staged(len(SCENES["box_diffuse_T"][0]), 4) and 17 <= clusters_of(len(SCENES["box_diffuse_T"][0])) <= 20


@pytest.mark.parametrize("name", sorted(SCENES))
def test_hit_share_is_on_the_side_the_note_says(name):
    tris, _, note = SCENES[name]
    share = rt.bounce_hit_share(tris)
    print(f"{name}: bounce_hit_share {share:.4f}")
    assert ("not hit-heavy" in note) == name.startswith("layers_")
    if "not hit-heavy" in note:
        assert share < WGS_HIT_SHARE
    else:
        assert share > WGS_HIT_SHARE


# ---- layers --------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    p = (a * b).astype(F)
    return ((p[..., 0] + p[..., 1]).astype(F) + p[..., 2]).astype(F)


def _cross(u, v):
    return np.stack([((u[..., 1] * v[..., 2]).astype(F) - (u[..., 2] * v[..., 1]).astype(F)).astype(F),
                     ((u[..., 2] * v[..., 0]).astype(F) - (u[..., 0] * v[..., 2]).astype(F)).astype(F),
                     ((u[..., 0] * v[..., 1]).astype(F) - (u[..., 1] * v[..., 0]).astype(F)).astype(F)], -1)


@functools.lru_cache(maxsize=None)
def floor_hits(n):
    """(launch pixel indices, primary hit points float32) of the frame's pixels whose primary ray ends on the floor."""
    name, W, H, _, _ = FRAMES[f"layers_{n}"]
    tris, cam, _ = SCENES[name]
    rays = launch_rays(cam, _cfg(W, H, 1, 4))
    rec, dst = hit_table(orc.ray_triangle, tris, rays)
    d = np.where(rec, dst, F(np.inf))
    win = np.argmin(d, 1)
    px = np.flatnonzero(rec.any(1) & (win >= len(tris) - 2))
    pos = np.stack([rays["pos"][c][px] for c in "xyz"], 1)
    dirs = np.stack([rays["dir"][c][px] for c in "xyz"], 1)
    return px, (pos + (dirs * d[px, win[px]][:, None]).astype(F)).astype(F)  # raytracing.c:238


@pytest.mark.parametrize("n", LAYERS)
def test_layers_clusters_are_oversized_and_reachable_from_the_floor(n):
    """With the grouping the library builds (scene_records_host, what an upload holds): cluster c is layer n - 1 - c -- the
    last one layer 0 and the floor --, every cluster carries ball_of's never-cull escape because a record of it has an edge
    above ED_RATIO_EDGE, and from every floor pixel's primary hit point every cluster has a record that the table mode's
    reach test keeps (the reference's float32 dot(AC, (p0 - A) x AB) > 0, raytracing.c:198-206).  So nLive = n there."""
    tris = SCENES[f"layers_{n}"][0]
    rec = rt.scene_records_host(tris)
    cl = rec["clTris"]
    idx = cl[:, 12].view(np.int32)
    assert len(idx) == 8 * n and sorted(idx) == list(range(8 * n))
    layer = np.concatenate([np.repeat(np.arange(n - 1, 0, -1), 8), np.zeros(6, np.int64), [0, 0]])  # the floor with layer 0
    assert np.array_equal(layer[idx].reshape(n, 8), np.repeat(np.arange(n - 1, -1, -1), 8).reshape(n, 8))
    assert set(idx[-8:]) >= {8 * n - 2, 8 * n - 1}
    assert len(rec["chunks"]) == (2 if n > CHUNK_CLUSTERS else 1)
    r = cl.view(F)
    A, AB, AC = r[:, 0:3], r[:, 3:6], r[:, 6:9]
    edge = np.sqrt((r[:, 3:9].astype(np.float64).reshape(-1, 2, 3) ** 2).sum(-1)).max(-1).reshape(n, 8)
    assert (edge.max(1) > ED_RATIO_EDGE).all()
    balls = rec["clusters"].view(F)
    assert np.isposinf(balls[:n, 4]).all(), "a cluster without the never-cull escape"
    assert (cl[:, 13] != 0).all(), "a stored normal that is not aligned (the reach test would keep it for that alone)"
    px, p0 = floor_hits(n)
    assert len(px) >= 100
    dac = _dot(AC[None], _cross((p0[:, None, :] - A[None]).astype(F), AB[None]))  # [pixels, records]
    live = (dac > 0).reshape(len(px), n, 8).any(-1)
    print(f"layers_{n}: {len(px)} floor pixels; reachable records per (pixel, cluster): min "
          f"{int((dac > 0).reshape(len(px), n, 8).sum(-1).min())}")
    assert live.all()


@pytest.mark.parametrize("n", LAYERS)
def test_layers_full_windows_keep_every_lane_alive(n):
    """Every state index S_0 .. S_63 of every floor pixel makes a first bounce (the floor's colour has a component 1), so
    the first window of a frame of 64 samples traces 64 live lanes at iteration 1: 64 n pairs, more than the list holds
    from n = 17 on, exactly the list for n = 16."""
    name, W, H, spp, mb = FRAMES[f"layers_{n}"]
    assert spp >= 64
    px, _ = floor_hits(n)
    hits, calls = state_samples(name, W, H, mb, tuple(int(p) for p in px), 0, 64)
    assert (calls >= 2).all()
    pairs = 64 * n
    assert (pairs > CHAIN_PAIRS) == (n >= 17) and (n != 16 or pairs == CHAIN_PAIRS)
    # the bounces end on different layers (a window's winners come from many clusters): hits per sample vary
    print(f"layers_{n}: hits per sample over the floor pixels' 64 state indices: {np.bincount(hits.reshape(-1))}")
    assert len(np.unique(hits)) >= 3


# ---- boxes ---------------------------------------------------------------------------------------------------------------
BOX_PIXELS = (0, 5, 100, 250, 333, 479)  # of the 24 x 20 frame


def test_box_diffuse_windows_pass_from_the_per_lane_loop_to_the_dense_cull():
    """box_diffuse_T, the first window of some pixel: at an iteration >= 2 more than 16 lanes are alive (per-lane loop: the
    HITS kernel's, without fusedG at 18 clusters) and at a later one between 1 and 16 (dense cull with nCl > 16)."""
    name, W, H, spp, mb = FRAMES["box_diffuse_T"]
    assert clusters_of(len(SCENES[name][0])) > DENSE_CULL_MAX and spp >= 64
    _, calls = state_samples(name, W, H, mb, BOX_PIXELS, 0, 64)
    found = 0
    for row in calls:
        alive = np.array([(row > i).sum() for i in range(mb + 1)])
        big = [i for i in range(2, mb + 1) if alive[i] > DENSE_CULL_MAX]
        small = [i for i in range(2, mb + 1) if 1 <= alive[i] <= DENSE_CULL_MAX]
        print(f"alive lanes by iteration: {alive.tolist()}")
        found += bool(big and small and max(small) > min(big))
        # a dense cull of more than 64 (lane, cluster) culls: the 64-at-a-time loop runs more than once
        assert any(alive[i] * 18 > 64 for i in small)
    assert found >= len(calls) // 2  # (the claim is that such windows exist; most pixels have one)


@pytest.mark.parametrize("frame", sorted(f for f in FRAMES if f.startswith(("box_mirror", "box_gloss")))
                         + [f"pass:{f}" for f in sorted(PASS_FRAMES) if f.startswith(("box_mirror", "box_gloss"))])
def test_shiny_boxes_make_exactly_max_bounce_hits(frame):
    if frame.startswith("pass:"):
        (name, W, H, mb), spp = PASS_FRAMES[frame[5:]], sum(PASS_SPLIT)
    else:
        name, W, H, spp, mb = FRAMES[frame]
    tris, cam, _ = SCENES[name]
    h = pr.hits_per_sample(tris, None, rt.default_scene(), cam, _cfg(W, H, spp, mb).desc())
    assert h.shape == (spp, W * H) and (h == mb).all(), f"{frame}: hits per sample {np.unique(h)}"
    # hq = mb hits move the walk mb lanes on: with mb >= 64 every window commits one sample (with 63, a
    # full window commits lanes 0 and 63)
    w = walk(lambda j: mb, spp)
    assert sum(c for _, _, c in w) == spp and max(c for _, _, c in w) <= 2
    if mb >= 64:
        assert len(w) == spp and [jn for jn, _, _ in w] == [mb * k for k in range(spp)]
    if name == "box_gloss":  # the samples differ (the mirror's do not: its path ignores the draws)
        d = _cfg(W, H, 1, mb).desc()
        rays = launch_rays(cam, _cfg(W, H, 1, mb))
        s0 = pr.seeds(d)
        rad0 = pr.sample(tris, None, rt.default_scene(), d, rays, s0)[0]
        rad1 = pr.sample(tris, None, rt.default_scene(), d, rays, pr.advance(s0, 7 * mb))[0]
        assert (rad0.view(np.uint32) != rad1.view(np.uint32)).any(1).mean() > 0.9


def test_deep_box_has_short_later_windows():
    """box_diffuse_deep (maxBounce 40, 130 samples): mixed hits per sample, several windows per pixel, and later windows
    whose nAct, from est = need * jn / k, is below 64."""
    name, W, H, spp, mb = FRAMES["box_diffuse_deep"]
    pixels = (0, 37, 64, 127)
    chunks: dict = {}

    def hits_of(p):
        def f(j):
            c = j // 256
            if (p, c) not in chunks:
                chunks[(p, c)] = state_samples(name, W, H, mb, (pixels[p],), 256 * c, 256)[0][0]
            return int(chunks[(p, c)][j % 256])
        return f

    short = 0
    for p in range(len(pixels)):
        w = walk(hits_of(p), spp)
        used = np.concatenate([chunks[(p, c)] for c in sorted(c for q, c in chunks if q == p)])
        print(f"pixel {pixels[p]}: windows (jn, nAct, samples) {w}; hits up to {int(used.max())}")
        assert len(w) >= 4 and sum(c for _, _, c in w) == spp
        short += any(n_act < 64 for _, n_act, _ in w[1:])
        assert used.min() == 1 and used.max() > 10
    assert short >= 1


# ---- the launches ---------------------------------------------------------------------------------------------------
def test_the_paths_meant_are_the_paths_taken():
    """tests/test_gpu_chain_paths.py's expected_report -- what each of its launches is held to through
    DeviceScene.chain_report -- spelled out for the launches these scenes exist for: a change of a scene or of a threshold
    that moves one of them off its path fails here."""
    e = expected_report
    for route in IN_KERNEL_SUMS:
        box = e("box_diffuse_T", route, False)  # the HITS kernel at 18 clusters: no fusedG
        assert box["hits"] and not box["general"] and box["chain_prim_f"] and box["wgs_per_cu"] == 4 and box["cluster_count"] == 18
        unstaged = e("box_primf_4", route, False)  # 21 clusters at 4 workgroups per CU: GENERAL for that alone
        assert unstaged["general"] and not unstaged["chain_prim_f"] and not unstaged["hits"] and unstaged["wgs_per_cu"] == 4
        below = e("box_primf_4_below", route, False)
        assert below["chain_prim_f"] and below["hits"] and not below["general"] and below["cluster_count"] == 20
        for n in (16, 17, 32):  # the plain kernel: fused table build at 16 live clusters, the separate build above
            lay = e(f"layers_{n}", route, False)
            assert not lay["general"] and not lay["hits"] and not lay["multi"] and lay["chain_prim_f"] and lay["wgs_per_cu"] == 3
        assert e("layers_33", route, False)["multi"] and e("layers_33", route, False)["chunk_count"] == 2
    assert not e("layers_32", "pipelined", False)["multi"] and e("layers_33", "pipelined", False)["general"]
    # without the cluster cull every live lane keeps every cluster: 64 nCl > 1024 pairs in a full window from 17 clusters on
    for name in ("layers_17", "layers_32", "box_diffuse_T", "box_primf_4"):
        assert 64 * e(name, "no_cluster_cull", False)["cluster_count"] > 1024
