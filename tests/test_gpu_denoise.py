"""The denoise kernels on the GPU (rtc_denoise_async, rt.denoise on device tensors; include/rtc.h): dOut and
dColors equal rtc_denoise_host byte for byte on every shape at which the kernels take another path, with every guide
subset and 1 .. 6 iterations, and on the designed values; dColors at byte offsets 0 .. 3; 64-byte canaries around dOut,
dColors and the scratch's stated size; the inputs unchanged.  One frame end to end: first hit, adaptive render and denoise
on device tensors against the same chain on the CPU references."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import denoise_reference as dr
import raytracingc_amd as rt
from raytracingc_amd import _abi
from raytracingc_amd._abi import RtcDenoiseDesc

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64  # bytes
POISON = 0xA5
SHAPES = dr.shapes(_abi.DENOISE_TILE_W, _abi.DENOISE_TILE_H)


def c_desc(d):
    return RtcDenoiseDesc(d.width, d.rows, d.iterations, d.flags, d.spp, d.normalSquarings, d.depthScale, d.colorScale,
                          d.albedoFloor)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared frames are read-only)


class DeviceFrame:
    """A frame's buffers on the device, uploaded once, and their host originals to compare with afterwards"""

    def __init__(self, frame):
        self.host = {k: np.ascontiguousarray(v) for k, v in frame.items() if isinstance(v, np.ndarray)}
        self.dev = {k: _dev(v) for k, v in self.host.items()}
        self.spp = frame["spp"]

    def unchanged(self, what):
        for k, v in self.host.items():
            assert np.array_equal(self.dev[k].cpu().numpy().view(np.uint8), v.view(np.uint8)), f"{what}: {k} changed"


def device_equals_host(df, d, subset, with_samples, offset, what, want_colors=True):
    """rtc_denoise_async on guarded buffers against rtc_denoise_host: dOut and dColors byte for byte, the guards intact."""
    import torch

    kw, _ = dr.guide_args(df.host, subset)
    want = rt.denoise(df.host["accum"], kw, df.host["samples"] if with_samples else None, d.spp if with_samples else None,
                      c_desc(d), colors=True)
    n = d.width * d.rows
    nbytes = rt.denoise_scratch_bytes(n, d.iterations)
    out = torch.full((GUARD + 12 * n + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    col = torch.full((GUARD + 4 + 3 * n + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    scratch = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0 and col.data_ptr() % 4 == 0 and scratch.data_ptr() % 16 == 0
    rt.denoise_async(df.dev["accum"].data_ptr(), df.dev["samples"].data_ptr() if with_samples else None, c_desc(d),
                     out.data_ptr() + GUARD, col.data_ptr() + GUARD + offset if want_colors else None,
                     scratch.data_ptr() + GUARD, nbytes, **{k + "_ptr": df.dev[k].data_ptr() for k in kw},
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, c, s = out.cpu().numpy(), col.cpu().numpy(), scratch.cpu().numpy()
    assert (o[:GUARD] == POISON).all() and (o[GUARD + 12 * n:] == POISON).all(), f"{what}: the guards around dOut"
    lo, hi = GUARD + offset, GUARD + offset + 3 * n
    assert (c[:lo] == POISON).all() and (c[hi:] == POISON).all(), f"{what}: the guards around dColors"
    assert (s[:GUARD] == POISON).all() and (s[GUARD + nbytes:] == POISON).all(), f"{what}: the guards around the scratch"
    got = o[GUARD:GUARD + 12 * n].view(np.uint32)
    ref = want[0].reshape(-1).view(np.uint32)
    diff = np.flatnonzero(got != ref)
    assert len(diff) == 0, (f"{what}: {len(diff)} differing words of {3 * n}, the first at {diff[:4]}: "
                            f"{got[diff[:4]].view(F)} for {ref[diff[:4]].view(F)}")
    if want_colors:
        assert np.array_equal(c[lo:hi], want[1].reshape(-1)), f"{what}: the Color bytes"
    else:
        assert (c == POISON).all(), f"{what}: dColors was not given"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_guide_subsets_and_iterations(shape, gpu_available):
    w, rows = shape
    df = DeviceFrame(dr.random_frame(w * 1000 + rows, w, rows))
    n = 0
    for si, subset in enumerate(dr.GUIDE_SUBSETS):
        flags = dr.guide_args(df.host, subset)[1]
        for it in range(1, 7):
            sq = (0, 1, 8)[(it + si) % 3]
            d = dr.desc(w, rows, it, flags, df.spp, sq, depth_scale=0.7, color_scale=1.5, albedo_floor=0.1)
            device_equals_host(df, d, subset, n % 2 == 1, n % 4, f"{w}x{rows} {subset} iterations {it} squarings {sq}",
                               want_colors=n % 5 != 4)
            n += 1
    df.unchanged(f"{w}x{rows}")


DESIGNED = dr.designed_frames()


@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_values(name, gpu_available):
    frame, dkw = DESIGNED[name]
    flags = dkw.get("flags", 0)
    rows, w = frame["accum"].shape[:2]
    df = DeviceFrame(frame)
    n = 0
    for subset in (("albedo",) if flags else ("none", "normal", "depth", "both")):
        for it in (1, 2, 3, 6):
            d = dr.desc(w, rows, it, spp=frame["spp"], **dkw)
            device_equals_host(df, d, subset, True, n % 4, f"{name} {subset} iterations {it}")
            device_equals_host(df, d, subset, False, (n + 2) % 4, f"{name} {subset} iterations {it}, no samples")
            n += 1
    df.unchanged(name)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_colors_at_every_byte_offset(offset, gpu_available):
    w, rows = 37, 9  # (3 * 333 bytes: odd, so the end is ragged at every offset)
    df = DeviceFrame(dr.random_frame(offset, w, rows))
    for it in (1, 2):
        d = dr.desc(w, rows, it, dr.DEMODULATE, df.spp, 1, depth_scale=0.7, color_scale=1.5, albedo_floor=0.1)
        device_equals_host(df, d, "albedo", True, offset, f"offset {offset} iterations {it}")


def test_python_denoise_on_tensors(gpu_available):
    import torch

    w, rows = 45, 38
    frame = dr.random_frame(5, w, rows)
    df = DeviceFrame(frame)
    d = rt.denoise_desc(w, rows, 4, 2, 0.7, 1.5, 0.1, True)
    guides = {k: frame[k] for k in ("normal", "depth", "albedo")}
    want = rt.denoise(frame["accum"], guides, frame["samples"], frame["spp"], d, colors=True)
    dguides = {k: df.dev[k] for k in guides}
    dguides["prim"] = torch.zeros((rows, w), dtype=torch.int32, device="cuda")
    got = rt.denoise(df.dev["accum"], dguides, df.dev["samples"], frame["spp"], d, colors=True)
    torch.cuda.synchronize()
    assert got[0].is_cuda and got[0].dtype == torch.float32 and got[1].dtype == torch.uint8
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    plain = rt.denoise(df.dev["accum"])  # (no guides, no samples, the default desc; no colors: a tensor alone)
    torch.cuda.synchronize()
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), rt.denoise(frame["accum"]).view(np.uint32))
    with pytest.raises(ValueError):
        rt.denoise(df.dev["accum"], {"normal": frame["normal"]})  # a host guide with a device accumulator
    df.unchanged("rt.denoise")


# ---- one frame end to end -----------------------------------------------------------------------------------------------
PIPELINE = dict(scene="ultracomplex", shape=(48, 40), spp=12, max_bounce=4, passes=(3, 3, 2, 2, 2), threshold=0.05,
                floor=0.02, capacity=128,
                desc=dict(iterations=4, normal_squarings=5, depth_scale=1.0, color_scale=0.05, albedo_floor=0.01,
                          flags=dr.DEMODULATE))


@functools.lru_cache(maxsize=None)
def pipeline_on_the_cpu():
    """The adaptive frame of tests/select_reference.py on tests/pixel_pass_reference.py, the first-hit buffers of
    tests/first_hit_reference.py, and rtc_denoise_host over them: (accum, samples, counts, guides, out, colors)"""
    import first_hit_reference as fh
    import pixel_pass_reference as ppr
    import select_reference as sr

    P = PIPELINE
    w, h = P["shape"]
    tris, sph, scene, cam, tonly = sr.frame_geometry(P["scene"])
    cfg = rt.RenderConfig(w, h, P["spp"], P["max_bounce"], bool(tonly))
    acc_k = ppr.per_sample(tris, sph, scene, cam, cfg.desc(), {})[0]
    _, counts, samples, accum = sr.adaptive_frame(acc_k, P["spp"], P["passes"], P["threshold"], P["floor"], P["capacity"])
    guides = fh.expected_for(tris, sph, tonly, cam, rt.RenderConfig(w, h, 0, 0, bool(tonly)))
    accum = np.ascontiguousarray(accum, F).reshape(h, w, 3)
    samples = np.ascontiguousarray(samples, np.int32).reshape(h, w)
    out, colors = rt.denoise(accum, guides, samples, P["spp"], c_desc(dr.desc(w, h, **P["desc"])), colors=True)
    return accum, samples, counts, guides, out, colors


def test_first_hit_adaptive_render_and_denoise_on_the_device(gpu_available):
    import select_reference as sr
    import torch

    P = PIPELINE
    w, h = P["shape"]
    accum, samples, counts, guides, want, want_colors = pipeline_on_the_cpu()
    print(f"pipeline: selections {counts}, sample counts {np.unique(samples).tolist()}")
    assert counts[0] > 0 and len(np.unique(samples)) >= 2  # (an adaptive frame: the pixels stopped at different counts)
    tris, sph, scene, cam, tonly = sr.frame_geometry(P["scene"])
    cfg = rt.RenderConfig(w, h, P["spp"], P["max_bounce"], bool(tonly))
    ds = rt.DeviceScene(tris, sph)
    try:
        dguides = {"depth": torch.zeros((h, w), dtype=torch.float32, device="cuda"),
                   "normal": torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"),
                   "albedo": torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")}
        st = torch.cuda.current_stream().cuda_stream
        ds.render_first_hit_async(cam, cfg, 0, dguides["depth"].data_ptr(), dguides["normal"].data_ptr(),
                                  dguides["albedo"].data_ptr(), stream=st)
        res = ds.render_adaptive_device(scene, cam, cfg, P["passes"], P["threshold"], P["floor"], P["capacity"])
        out, colors = rt.denoise(res["accum"], dguides, res["samples"], P["spp"], c_desc(dr.desc(w, h, **P["desc"])),
                                 colors=True)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        got_guides = {k: v.cpu().numpy() for k, v in dguides.items()}
        out, colors = out.cpu().numpy(), colors.cpu().numpy()
    finally:
        torch.cuda.synchronize()
        ds.close()
    for k, v in got_guides.items():
        assert np.array_equal(v.view(np.uint32), np.ascontiguousarray(guides[k]).view(np.uint32)), k
    assert got["counts"].tolist() == counts and np.array_equal(got["samples"], samples)
    assert np.array_equal(got["accum"].view(np.uint32), accum.view(np.uint32))
    assert int((out.view(np.uint32) != want.view(np.uint32)).sum()) == 0
    assert np.array_equal(colors, want_colors)
    # the denoised frame is not the resolved one: the filter did something
    assert (colors != got["colors"]).any()
