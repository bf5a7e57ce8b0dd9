"""Whole frames of the material scenes (tests/material_scenes.py: smoothness -1 .. 3e38, colours 0, -0, above 1, negative,
NaN and inf, emission 3e38) on every route of the renderer, against the CPU oracle -- which tests/test_oracle.py pins to the
reference's own calcColor at these values: NaN positions equal, every other float of the accumulator bit-equal, the u8 frame
equal, the segment count equal where the launch counts.  Bit comparisons, no tolerance.  The routes, the report check and
compare() are tests/test_gpu_chain_paths.py's; what the lanes do at these values (which of them are beyond the cull's
|dir|_1 <= 4, which paths the roulette ends) follows from the oracle alone in tests/test_material_scenes.py.

The gate itself shows in no frame -- culls that ignored it would still lose no hit -- but in the work counters: a ray
beyond the bound visits every triangle (test_rays_beyond_the_bound_visit_every_triangle).

Beside the frames: two passes split inside a window (inf and NaN accumulators stored and reloaded), a refit to non-finite
materials (the records keep every bit, NaN payloads and zero signs included), three pipelined frames around a blinding one
(no inf or NaN leaks through a deferred slot or a merged sky word), and the sphere scenes -- a blinding and a nonfinite
sphere among them -- on the split launch, on the one-lane-per-pixel kernel and in two passes."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import progressive_reference as pr
import raytracingc_amd as rt
from chain_path_scenes import PASS_SPLIT
from material_scenes import FRAMES, ORDINARY, PASS_FRAMES, SCENES, SPHERE_FRAME, SPHERE_NAMES, sky, sphere_scene
from test_gpu_chain_paths import NO_GEOMETRY_KERNEL, ROUTES, check_report, compare, expected_report

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(frame):
    """The oracle's (u8, floats, segments) of the frame, computed once and left unchanged."""
    scene_name, W, H, spp, mb = FRAMES[frame]
    tris, cam, _ = SCENES[scene_name]
    col, acc, seg = orc.render(tris, None, sky(frame), cam, rt.RenderConfig(W, H, spp, mb, True).desc(), threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


@functools.lru_cache(maxsize=None)
def _device_scene(scene_name):
    return rt.DeviceScene(SCENES[scene_name][0], None)


def _buffers(H, W, counters):
    import torch

    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
    torch.cuda.synchronize()
    return out, acc, seg


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_frame_matches_oracle(frame, route, gpu_available):
    import torch

    scene_name, W, H, spp, mb = FRAMES[frame]
    cam, scene = SCENES[scene_name][1], sky(frame)
    cfg = rt.RenderConfig(W, H, spp, mb, True, **ROUTES[route])
    ocol, oacc, oseg = _oracle(frame)
    ds = _device_scene(scene_name)
    st = torch.cuda.current_stream().cuda_stream
    for counters in (False, True):
        out, acc, seg = _buffers(H, W, counters)
        before = ds.chain_report()
        ds.render_rows_async(scene, cam, cfg, out.data_ptr(), acc.data_ptr(), seg.data_ptr() if counters else None, st)
        torch.cuda.synchronize()
        what = f"{frame} {route} counters={counters}"
        if route in NO_GEOMETRY_KERNEL:
            assert ds.chain_report() == before, what
        else:
            check_report(ds, before, expected_report(scene_name, route, counters, scenes=SCENES), what)
        compare(what, out.cpu().numpy(), acc.cpu().numpy(), ocol, oacc)
        if counters:
            assert int(seg.cpu().numpy()[0]) == oseg, f"{what}: segments"


# ---- the gate, by the work counters ---------------------------------------------------------------------------------------
GATE_FRAMES = ("boxT_s8", "fine_s8", "fine_s2p5", "boxT_s1e6")


@pytest.mark.parametrize("frame", GATE_FRAMES)
def test_rays_beyond_the_bound_visit_every_triangle(frame, gpu_available):
    """The frames cannot show the |dir|_1 <= 4 gate: a cull that ignored it would, by the argument in
    tests/test_material_scenes.py, still never lose a hit.  The work counters can.  A ray beyond the bound is culled nowhere
    -- not by a cluster's ball, not by a chunk's, not by the first bounce's table of records reachable from the primary
    hit point, which the wave's ballot drops -- so it visits every triangle of the scene: with B and I the accumulated
    samples' bounce calls beyond and within the bound (the oracle's recorded paths), the launch's ray-triangle tests,
    less those of the same launch at maxBounce 1 (the primary rays'), lie in [T B, T (B + I)], and are T (B + I)
    exactly without the cluster cull.  A library whose culls ignore the gate counts 14,288,352 < T B = 14,334,480 on
    boxT_s8 and fails fine_s8 and fine_s2p5 as well; one whose table ignores the ballot fails boxT_s8 and boxT_s1e6 (the
    table leaves out the records of the primary hit's own wall); both render every frame of this module right.
    The limit of this test: a launch that counts runs the GENERAL instantiation, so the gates of the HITS kernel -- fusedG's
    and its per-lane loop's, which the in-kernel-sum routes of the hit-heavy boxes run -- are held by no counter, and by no
    frame either: a library with rhoOk removed there alone passes every test."""
    import torch

    from test_material_scenes import frame_paths, rho_of

    scene_name, W, H, spp, mb = FRAMES[frame]
    tris, cam, _ = SCENES[scene_name]
    calls, ncalls, _ = frame_paths(frame)
    bounce = np.arange(calls.shape[2])[None, None, :] < ncalls[..., None]
    bounce[..., 0] = False
    with np.errstate(invalid="ignore"):
        within = bounce & (rho_of(calls["dir"]) <= np.float32(4.0))
    B, I, T = int((bounce & ~within).sum()), int(within.sum()), len(tris)
    assert B >= 500 and (I >= 500 or frame.endswith("_s1e6"))
    ds = _device_scene(scene_name)
    st = torch.cuda.current_stream().cuda_stream
    for route in ("joined_deferred", "joined_inline", "hoisted", "no_cluster_cull"):
        tests = []
        for bounces in (mb, 1):
            out, _, seg = _buffers(H, W, True)
            cfg = rt.RenderConfig(W, H, spp, bounces, True, **ROUTES[route])
            ds.render_rows_async(sky(frame), cam, cfg, out.data_ptr(), None, seg.data_ptr(), st)
            torch.cuda.synchronize()
            tests.append(int(seg.cpu().numpy()[2]))
        got = tests[0] - tests[1]
        print(f"{frame} {route}: {got} bounce-ray triangle tests; T B = {T * B}, T (B + I) = {T * (B + I)}")
        if route == "no_cluster_cull":
            assert got == T * (B + I), f"{frame} {route}"
        else:
            assert T * B <= got <= T * (B + I), f"{frame} {route}: a ray beyond the bound skipped triangles"


# ---- spheres ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere_oracle(name):
    tris, sph, cam, _ = sphere_scene(name)
    W, H, spp, mb = SPHERE_FRAME
    col, acc, seg = orc.render(tris, sph, rt.default_scene(), cam, rt.RenderConfig(W, H, spp, mb, False).desc(), threads=16)
    col.setflags(write=False)
    acc.setflags(write=False)
    return col, acc, seg


@functools.lru_cache(maxsize=None)
def _sphere_device_scene(name):
    tris, sph, _, _ = sphere_scene(name)
    return rt.DeviceScene(tris, sph)


SPHERE_ROUTES = {"split": dict(split_spheres=True), "auto": {}, "nocoop": dict(coop=False),
                 "split_inline": dict(split_spheres=True, chain_inline=True), "split_hoisted": dict(split_spheres=True, hoist=True),
                 "split_no_cluster_cull": dict(split_spheres=True, cluster_cull=False)}


@pytest.mark.parametrize("route", sorted(SPHERE_ROUTES))
@pytest.mark.parametrize("name", SPHERE_NAMES)
def test_sphere_frame_matches_oracle(name, route, gpu_available):
    """Sphere materials from the same lists, one sphere per kind (bright with smoothness 2.5, negative with 8, a blinding
    lamp, a bright ground, a zero; in spheres_nonfinite a NaN and an inf component and emission inf), through KLOAD(spheres)
    at the primary hit and P.spheres[] later: +inf and NaN pixels in every frame (tests/test_material_scenes.py counts them).  The path taken is read as tests/test_gpu_sphere_split.py reads
    it -- kernel_times() reports the split launch's kernels only when a launch took it -- and the default routing is the
    upload gate's, which follows the host probe's share (at most 0.5: split)."""
    import torch

    tris, sph, cam, _ = sphere_scene(name)
    W, H, spp, mb = SPHERE_FRAME
    ocol, oacc, oseg = _sphere_oracle(name)
    ds = _sphere_device_scene(name)
    share = rt.bounce_hit_share(tris, sph)
    assert np.isfinite(share) and ds.sphere_split == (share <= 0.5) == (name != "spheres_closed")
    kw = SPHERE_ROUTES[route]
    cfg = rt.RenderConfig(W, H, spp, mb, False, **kw)
    split = kw.get("coop", True) and (kw.get("split_spheres", False) or ds.sphere_split)
    st = torch.cuda.current_stream().cuda_stream
    ds.set_timing(True)
    try:
        for counters in (True, False):
            out, acc, seg = _buffers(H, W, counters)
            ds.render_rows_async(rt.default_scene(), cam, cfg, out.data_ptr(), acc.data_ptr(),
                                 seg.data_ptr() if counters else None, st)
            torch.cuda.synchronize()
            what = f"{name} {route} counters={counters}"
            assert (ds.kernel_times() is not None) == split, f"{what}: the launch took the other path"
            compare(what, out.cpu().numpy(), acc.cpu().numpy(), ocol, oacc)
            if counters:
                assert int(seg.cpu().numpy()[0]) == oseg, f"{what}: segments"
    finally:
        ds.set_timing(False)


# ---- two passes, split inside a window -------------------------------------------------------------------------------------
PASSES = sorted(PASS_FRAMES) + ["spheres_open", "spheres_nonfinite"]


@functools.lru_cache(maxsize=None)
def _pass_reference(frame):
    """progressive_reference's chain over PASS_SPLIT and the whole frame's oracle: (chain, (u8, floats, segments))."""
    if frame.startswith("spheres_"):
        tris, sph, cam, _ = sphere_scene(frame)
        W, H, _, mb = SPHERE_FRAME
        scene, tonly = rt.default_scene(), False
    else:
        scene_name, W, H, mb = PASS_FRAMES[frame]
        (tris, cam, _), sph, scene, tonly = SCENES[scene_name], None, sky(frame), True
    d = rt.RenderConfig(W, H, sum(PASS_SPLIT), mb, tonly).desc()
    ch = pr.chain(tris, sph, scene, cam, d, list(PASS_SPLIT), {})
    whole = orc.render(tris, sph, scene, cam, d, threads=16)
    for a in [x for t in ch for x in t[1:4]] + list(whole[:2]):
        a.setflags(write=False)
    return ch, whole, (W, H, mb, cam, scene, tonly)


def _same_floats(a, want):
    """Differing words of two float arrays given as uint32: NaN against NaN counts as equal (a NaN's sign may differ
    between gfx950 and x86), NaN against a number does not."""
    fa, fw = a.view(np.float32), want.view(np.float32)
    return int(((a != want) & ~(np.isnan(fa) & np.isnan(fw))).sum())


@pytest.mark.parametrize("route", ["joined_deferred", "joined_inline", "hoisted"])
@pytest.mark.parametrize("frame", PASSES)
def test_two_passes_match_the_reference(frame, route, gpu_available):
    """37 + 27 samples: after each pass the accumulator (inf and NaN included: stored by the first pass, reloaded by the
    second), the u8 frame and the RNG states are the progressive reference's; the sum is the one-launch oracle's."""
    import torch

    ch, (ocol, oacc, oseg), (W, H, mb, cam, scene, tonly) = _pass_reference(frame)
    spp = sum(PASS_SPLIT)
    kw = dict(ROUTES[route], split_spheres=True) if frame.startswith("spheres_") else ROUTES[route]
    cfg = rt.RenderConfig(W, H, spp, mb, tonly, **kw)
    ds = _sphere_device_scene(frame) if frame.startswith("spheres_") else _device_scene(PASS_FRAMES[frame][0])
    st = torch.cuda.current_stream().cuda_stream
    for counters in (False, True):
        col = torch.full((H, W, 3), 0xFF, dtype=torch.uint8, device="cuda")
        acc = torch.full((H, W, 3), -1, dtype=torch.int32, device="cuda")  # 0xFF bytes
        rng = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        seg = torch.zeros(rt.RTC_SEGMENT_COUNTERS, dtype=torch.int64, device="cuda") if counters else None
        done = 0
        for count, (rdone, racc, rrng, rcol, _) in zip(PASS_SPLIT, ch):
            torch.cuda.synchronize()
            before = ds.chain_report()
            ds.render_samples_async(scene, cam, cfg, done, count, col.data_ptr(), acc.data_ptr(), rng.data_ptr(),
                                    seg.data_ptr() if counters else None, st)
            torch.cuda.synchronize()
            done += count
            what = f"{frame} {route} counters={counters} after {done}/{spp}"
            if frame.startswith("spheres_"):
                rep = ds.chain_report()
                assert rep["launches"] == before["launches"] + 1 and rep["spheres"] and rep["resume"], what
            else:
                check_report(ds, before, expected_report(PASS_FRAMES[frame][0], route, counters, resume=True, scenes=SCENES),
                             what)
            a, s, c = acc.cpu().numpy().view(np.uint32), rng.cpu().numpy().view(np.uint32), col.cpu().numpy()
            bad = _same_floats(a, _bits(racc)), int((s != rrng).sum()), int((c != rcol).sum())
            assert done == rdone and bad == (0, 0, 0), f"{what}: differing accumulator words, states, colour bytes {bad}"
        compare(f"{frame} {route} counters={counters}: the oracle's frame", c, a.view(np.float32), ocol, oacc)
        if counters:
            assert int(seg.cpu().numpy()[0]) == oseg, f"{frame} {route}: segments"


# ---- refit ----------------------------------------------------------------------------------------------------------------
def _payload_nans(tris):
    """A copy whose NaNs carry payloads and signs: a copy that went through arithmetic would lose them."""
    t = tris.copy()
    m = t["mat"]
    nan = np.flatnonzero(np.isnan(m["color"]["x"]))
    assert len(nan) >= 3
    for i, word in zip(nan, (0x7FC12345, 0xFFC00001, 0x7FFFFFFF)):
        m["color"]["x"][i:i + 1] = np.array([word], np.uint32).view(np.float32)
    i = int(np.flatnonzero(np.isnan(m["emissionStrength"]))[0])
    m["emissionStrength"][i:i + 1] = np.array([0xFFFFFFFF], np.uint32).view(np.float32)
    return t


def test_refit_copies_materials_bit_for_bit(gpu_available):
    """box_diffuse_T's geometry with ordinary materials, updated in place to the nonfinite materials and then to smoothness
    2.5: each frame afterwards is the oracle's, and the material records the refit kernel wrote (DeviceScene.records, the
    probe of tests/test_gpu_scene_update.py) are the input's five floats bit for bit -- NaN payload, NaN sign and the sign
    of zero included -- and the host statement's."""
    import torch

    plain = ORDINARY["cbox_nonfinite"]
    odd = _payload_nans(SCENES["cbox_nonfinite"][0])
    zero = SCENES["cbox_zero"][0]
    steep = SCENES["boxT_s2p5"][0]
    assert len(plain) == len(odd) == len(steep) == len(zero)
    st = torch.cuda.current_stream().cuda_stream
    ds = rt.DeviceScene(plain, None)
    try:
        for frame, tris in (("cbox_nonfinite", odd), ("cbox_zero", zero), ("boxT_s2p5", steep)):
            scene_name, W, H, spp, mb = FRAMES[frame]
            cam = SCENES[scene_name][1]
            ds.update(tris=tris)
            rec, host = ds.records(), rt.scene_records_host(plain, tris)
            want = np.stack([tris["mat"]["color"][c] for c in "xyz"] + [tris["mat"]["emissionStrength"],
                                                                        tris["mat"]["smoothness"]], 1).view(np.uint32)
            assert np.array_equal(rec["mats"][:len(tris), :5], want), f"{frame}: the material records differ from the input"
            assert np.array_equal(rec["mats"], host["mats"]), f"{frame}: the material records differ from the host statement"
            col, acc, seg = orc.render(tris, None, sky(frame), cam, rt.RenderConfig(W, H, spp, mb, True).desc(), threads=16)
            for kw in (dict(), dict(chain_inline=True), dict(coop=False)):
                out, a, s = _buffers(H, W, True)
                ds.render_rows_async(sky(frame), cam, rt.RenderConfig(W, H, spp, mb, True, **kw), out.data_ptr(), a.data_ptr(),
                                     s.data_ptr(), st)
                torch.cuda.synchronize()
                compare(f"after the update to {frame} {kw}", out.cpu().numpy(), a.cpu().numpy(), col, acc)
                assert int(s.cpu().numpy()[0]) == seg, f"after the update to {frame} {kw}: segments"
    finally:
        ds.close()


# ---- pipelined ------------------------------------------------------------------------------------------------------------
def test_pipelined_frames_around_a_blinding_one(gpu_available):
    """Three overlapped launches on two alternating buffers -- ordinary materials, blinding, ordinary again --, an update
    before each: every frame equals its own oracle, so no inf or NaN of the middle frame leaks into the last one through a
    deferred slot, a merged sky word or the buffer the first frame used."""
    import torch

    scene_name, W, H, spp, mb = FRAMES["cbox_blinding"]
    cam, scene = SCENES[scene_name][1], sky("cbox_blinding")
    geoms = [ORDINARY[scene_name], SCENES[scene_name][0], ORDINARY[scene_name]]
    d = rt.RenderConfig(W, H, spp, mb, True).desc()
    want = [orc.render(g, None, scene, cam, d, threads=16) for g in geoms[:2]]
    want.append(want[0])
    assert np.isnan(want[1][1]).any() and np.isinf(want[1][1]).any() and np.isfinite(want[0][1]).all()
    cfg = rt.RenderConfig(W, H, spp, mb, True, overlap=True)
    dev = [torch.from_numpy(g.copy().view(np.uint8)).cuda() for g in geoms]
    ds = rt.DeviceScene(geoms[0], None)
    st, cp = torch.cuda.Stream(), torch.cuda.Stream()
    cols = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    accs = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    freed, got = [None, None], []
    try:
        for k in range(3):
            b = k % 2
            if freed[b] is not None:  # buffer b is rewritten only after its previous frame was copied
                st.wait_event(freed[b])
            ds.update(tris=dev[k], stream=st.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(st)  # (a torch event has no hipEvent_t until its first record)
            ds.set_frame_event(ev.cuda_event)
            ds.render_rows_async(scene, cam, cfg, cols[b].data_ptr(), accs[b].data_ptr(), None, st.cuda_stream)
            cp.wait_event(ev)
            with torch.cuda.stream(cp):
                got.append((cols[b].clone(), accs[b].clone()))
                freed[b] = torch.cuda.Event()
                freed[b].record(cp)
        torch.cuda.synchronize()
        for k, (c, a) in enumerate(got):
            compare(f"pipelined frame {k}", c.cpu().numpy(), a.cpu().numpy(), want[k][0], want[k][1])
    finally:
        torch.cuda.synchronize()
        ds.close()
