"""The ray order on the GPU (include/rtc.h): the device's keys are rtc_ray_keys_host's byte for byte, the
device's order is numpy's stable argsort of them at every size where the sort takes another path, nothing is written
outside the stated buffers, gather and scatter are numpy's indexing, and the three queries give the same words through an
order as without one.  The key's statement and the designed sets are tests/ray_order_reference.py's, checked without a GPU
by tests/test_ray_order_reference.py; the paths' oracle is tests/trace_paths_reference.py's."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ray_order_reference as ro
import raytracingc_amd as rt
import trace_paths_reference as tp
import trace_rays_reference as tr
from conftest import load_tris
from primary_rays import launch_rays
from raytracingc_amd import _abi

pytestmark = pytest.mark.gpu

B = _abi.RAY_ORDER_KEYS_PER_GROUP  # keys per sort workgroup
G = _abi.RAY_ORDER_SCAN_GROUPS     # workgroup counts per step of a scan workgroup's loop
SIZES = [1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, G * B + 1]
GUARD = 0x5A5A5A5A
GUARD_WORDS = 64
SCENE = rt.default_scene()
WAVE = rt.RTC_F_WAVE_PER_RAY
QUERY_SCENES = ("default", "ultracomplex", "layers_33")  # box and sphere; the flagship; 33 clusters in two chunks


@functools.lru_cache(maxsize=None)
def _geometry(name):
    if name == "ultracomplex":
        return load_tris("ultracomplex")[0], None, 1, rt.camera_basis()
    return tr.geometry(name)


@functools.lru_cache(maxsize=None)
def _scene(name):
    tris, spheres = _geometry(name)[:2]
    return rt.DeviceScene(tris, spheres)


def _dev(rays):
    """The rays as a float32 [n, 6] tensor on the device."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6).copy()).cuda()


def _words(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


@functools.lru_cache(maxsize=None)
def _pool(n):
    """n rays in the box LO, HI: the designed origins and directions first, then seeded random rays whose origins fall into
    few cells (long runs of equal keys among many distinct ones)."""
    head = np.concatenate([ro.origin_set(), ro.direction_set()])
    if n <= len(head):
        out = head[:n].copy()
    else:
        rng = np.random.default_rng(n)
        m = n - len(head)
        ext = (ro.HI - ro.LO).astype(np.float64)
        pos = ro.LO + ext * rng.integers(0, 8, (m, 3)) / 8.0 + ext / 64
        dirs = rng.normal(size=(m, 3))
        dirs[rng.random(m) < 0.3] = [0.1, 0.2, 0.9]  # ties in the direction bits as well
        out = np.concatenate([head, ro.make_rays(pos.astype(np.float32), dirs.astype(np.float32))])
    out.setflags(write=False)
    return out


def _sort_on_device(rays, lo, hi, want_keys=True):
    """rtc_ray_order_async on guarded buffers: (order uint32 [n], keys uint32 [n] or None); asserts the guards after the
    order, the keys and the scratch's stated size, and that the rays are as they were."""
    import torch

    n = len(rays)
    ds = _scene("default")
    d = _dev(rays)
    before = d.clone()
    nbytes = rt.ray_order_scratch_bytes(n)
    assert nbytes % 16 == 0
    order = torch.full((n + GUARD_WORDS,), GUARD, dtype=torch.int32, device="cuda")
    keys = torch.full((n + GUARD_WORDS,), GUARD, dtype=torch.int32, device="cuda") if want_keys else None
    scratch = torch.full((nbytes // 4 + GUARD_WORDS,), GUARD, dtype=torch.int32, device="cuda")
    assert scratch.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ds.ray_order_async(d.data_ptr(), n, order.data_ptr(), scratch.data_ptr(), nbytes, (lo, hi),
                       keys.data_ptr() if want_keys else 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = order.cpu().numpy().view(np.uint32)
    assert (o[n:] == GUARD).all(), "words after dOrder were written"
    assert (scratch[nbytes // 4:].cpu().numpy().view(np.uint32) == GUARD).all(), "words after the scratch were written"
    assert torch.equal(d.view(torch.int32), before.view(torch.int32)), "the rays were written"
    k = None
    if want_keys:
        k = keys.cpu().numpy().view(np.uint32)
        assert (k[n:] == GUARD).all(), "words after dKeys were written"
        k = k[:n]
    return o[:n], k


@pytest.mark.parametrize("name", sorted(ro.DESIGNED))
def test_device_keys_equal_the_host_statement(name, gpu_available):
    make, lo, hi = ro.DESIGNED[name]
    rays = make()
    want = rt.ray_keys_host(rays, lo, hi)
    order, keys = _sort_on_device(rays, lo, hi)
    bad = np.flatnonzero(keys != want)
    print(f"{name}: {len(rays)} rays, {len(bad)} keys differ")
    assert len(bad) == 0, (rays[bad[:4]], keys[bad[:4]], want[bad[:4]])
    assert np.array_equal(order, np.argsort(want, kind="stable"))


@pytest.mark.parametrize("n", SIZES)
def test_order_is_the_stable_argsort(n, gpu_available):
    rays = _pool(n)
    want = rt.ray_keys_host(rays, ro.LO, ro.HI)
    order, keys = _sort_on_device(rays, ro.LO, ro.HI, want_keys=n % 2 == 1)  # (dKeys is nullable: the even sizes omit it)
    expect = np.argsort(want, kind="stable").astype(np.uint32)
    bad = np.flatnonzero(order != expect)
    print(f"n {n}: {len(np.unique(want))} distinct keys, {len(bad)} places differ")
    assert keys is None or np.array_equal(keys, want)
    assert len(bad) == 0, (bad[:8], order[bad[:8]], expect[bad[:8]])


def _patterns():
    n = 2 * B + 1
    i = np.arange(n, dtype=np.int64)
    low = [v for v in range(256) if (v & 63) <= 58]  # bottom digits whose px, py bins can both be met (px + py <= 1)
    cells = (np.arange(256, dtype=np.int64) * 97) % 32768
    return {
        "all_equal": np.full(n, 5 << 15 | 3 << 12 | 7 << 6 | 9, np.int64),
        "descending": ((n - 1 - i) // 31 << 15) | ((n - 1 - i) % 31),
        "top_digit": ((i * 37) % 64) << 24 | 0x123 << 12 | 0x145,
        "bottom_digit": np.array(low, np.int64)[(i * 37) % len(low)] | 0x2345 << 15,
        "ties_in_256_cells": cells[(i // 7) % 256] << 15 | 2 << 12,
    }


@pytest.mark.parametrize("pattern", ["all_equal", "descending", "top_digit", "bottom_digit", "ties_in_256_cells"])
def test_key_patterns(pattern, gpu_available):
    wanted = _patterns()[pattern].astype(np.uint32)
    n = len(wanted)
    rays = ro.rays_with_keys(wanted)
    assert np.array_equal(rt.ray_keys_host(rays, ro.LO, ro.HI), wanted)
    order, keys = _sort_on_device(rays, ro.LO, ro.HI)
    assert np.array_equal(keys, wanted)
    assert np.array_equal(order, np.argsort(wanted, kind="stable"))
    if pattern == "all_equal":
        assert np.array_equal(order, np.arange(n))
    if pattern == "descending":
        assert (np.diff(wanted.astype(np.int64)) < 0).all() and np.array_equal(order, np.arange(n)[::-1])
    if pattern == "ties_in_256_cells":
        assert len(np.unique(wanted)) == 256


@pytest.mark.parametrize("n", [1, 65, 2 * B + 1])
@pytest.mark.parametrize("elem_bytes", [1, 4, 12, 24, 64])
def test_gather_and_scatter(elem_bytes, n, gpu_available):
    """gather equals numpy's indexing, scatter(gather(x)) == x, and the bytes around both destinations stay; single bytes
    from and to odd addresses."""
    import torch

    rng = np.random.default_rng(elem_bytes * 100003 + n)
    x = rng.integers(0, 256, (n, elem_bytes), dtype=np.uint8)
    perm = rng.permutation(n).astype(np.int32)
    pad = 257 if elem_bytes == 1 else 256
    st = torch.cuda.current_stream().cuda_stream

    def guarded(fill=None):
        t = torch.full((2 * pad + n * elem_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        if fill is not None:
            t[pad:pad + n * elem_bytes] = torch.from_numpy(fill.reshape(-1)).cuda()
        return t

    src, mid, back = guarded(x), guarded(), guarded()
    order = torch.from_numpy(perm).cuda()
    assert (src.data_ptr() + pad) % 2 == (1 if elem_bytes == 1 else 0)
    torch.cuda.synchronize()
    rt.gather_async(mid.data_ptr() + pad, src.data_ptr() + pad, order.data_ptr(), n, elem_bytes, st)
    rt.scatter_async(back.data_ptr() + pad, mid.data_ptr() + pad, order.data_ptr(), n, elem_bytes, st)
    torch.cuda.synchronize()
    for t, want, what in ((mid, x[perm], "gather"), (back, x, "scatter of the gather"), (src, x, "the source")):
        h = t.cpu().numpy()
        assert (h[:pad] == 0xA5).all() and (h[pad + n * elem_bytes:] == 0xA5).all(), f"{what}: bytes around it were written"
        assert np.array_equal(h[pad:pad + n * elem_bytes].reshape(n, elem_bytes), want), what


def test_scene_bounds_and_both_entries(gpu_available):
    """bounds() is the box of the vertices and the sphere's extent; the host twin, the tensor path and the stable argsort of
    the host keys in that box agree; an update does not move the box."""
    for name in ("default", "ultracomplex"):
        tris, spheres = _geometry(name)[:2]
        v = np.concatenate([np.stack([tris[k][c] for c in "xyz"], 1) for k in ("posA", "posB", "posC")]).astype(np.float32)
        lo, hi = v.min(0), v.max(0)
        if spheres is not None and len(spheres):
            c = np.stack([spheres["pos"][k] for k in "xyz"], 1).astype(np.float32)
            r = spheres["r"].astype(np.float32)[:, None]
            lo, hi = np.minimum(lo, (c - r).min(0)), np.maximum(hi, (c + r).max(0))
        ds = _scene(name)
        got_lo, got_hi = ds.bounds()
        assert np.array_equal(got_lo, lo) and np.array_equal(got_hi, hi), name
        rays = _query_rays(name)[0]
        want_keys = rt.ray_keys_host(rays, lo, hi)
        want = np.argsort(want_keys, kind="stable")
        order, keys = ds.ray_order(rays, keys=True)
        assert order.dtype == np.uint32 and np.array_equal(order, want) and np.array_equal(keys, want_keys)
        t_order, t_keys = ds.ray_order(_dev(rays), keys=True)
        assert t_order.is_cuda and np.array_equal(t_order.cpu().numpy(), want)
        assert np.array_equal(t_keys.cpu().numpy().view(np.uint32), want_keys)
        other = ds.ray_order(rays, bounds=(ro.LO, ro.HI))
        assert np.array_equal(other, np.argsort(rt.ray_keys_host(rays, ro.LO, ro.HI), kind="stable"))
    tris = tr.geometry("chunks")[0]
    moved = tris.copy()
    moved["posA"]["x"] += np.float32(3)
    ds = rt.DeviceScene(tris, None)
    try:
        before = ds.bounds()
        ds.update(tris=moved)
        after = ds.bounds()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        ds.close()


@functools.lru_cache(maxsize=None)
def _query_rays(name):
    """(rays, seeds, limits): the scene's camera frame at 96 x 54 in a seeded permutation, then 512 seeded bounce-like rays
    from points on the triangles (direction = normal + a random unit vector, the reference's diffuse lobe); hashed seeds;
    limits around the distances that occur, some infinite."""
    tris, _, tonly, cam = _geometry(name)
    rng = np.random.default_rng(len(name) + 2024)
    cam_rays = launch_rays(cam, rt.RenderConfig(96, 54, 0, 0, bool(tonly)))
    cam_rays = cam_rays[rng.permutation(len(cam_rays))]
    t = tris[rng.integers(0, len(tris), 512)]
    vert = lambda k: np.stack([t[k][c] for c in "xyz"], 1).astype(np.float64)  # noqa: E731
    u, v = rng.random((512, 1)), rng.random((512, 1))
    flip = (u + v) > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    pos = vert("posA") + u * (vert("posB") - vert("posA")) + v * (vert("posC") - vert("posA"))
    w = rng.normal(size=(512, 3))
    dirs = vert("normal") + w / np.linalg.norm(w, axis=1, keepdims=True)
    rays = np.concatenate([cam_rays, ro.make_rays(pos.astype(np.float32), dirs.astype(np.float32))])
    lim = (10.0 ** rng.uniform(-1, 1.5, len(rays))).astype(np.float32)
    lim[rng.random(len(rays)) < 0.1] = np.inf
    seeds = tp.hash_seeds(len(rays))
    for a in (rays, lim):
        a.setflags(write=False)
    return rays, seeds, lim


@pytest.mark.parametrize("name", QUERY_SCENES)
def test_trace_rays_through_an_order(name, gpu_available):
    ds, tonly = _scene(name), bool(_geometry(name)[2])
    rays = _query_rays(name)[0]
    plain = ds.trace_rays(_dev(rays), tonly)
    assert (plain["prim"] != -1).any() and (name == "default" or (plain["prim"] == -1).any()), "hits (and misses: the box is closed)"
    for what, got in (("tensor", ds.trace_rays(_dev(rays), tonly, order=True)),
                      ("numpy", ds.trace_rays(rays, tonly, order=True)),
                      ("precomputed", ds.trace_rays(_dev(rays), tonly, order=ds.ray_order(rays)))):
        for k in ("prim", "depth", "normal", "albedo"):
            assert np.array_equal(got[k].view(np.uint32), plain[k].view(np.uint32)), (name, what, k)


@pytest.mark.parametrize("name", QUERY_SCENES)
def test_occluded_through_an_order(name, gpu_available):
    ds, tonly = _scene(name), bool(_geometry(name)[2])
    rays, _, lim = _query_rays(name)
    plain, count = ds.occluded(_dev(rays), lim, tonly, count=True)
    assert 0 < count < len(rays) and count == int(plain.sum())
    import torch

    lim_t = torch.from_numpy(lim.copy()).cuda()
    for what, (got, c) in (("tensor", ds.occluded(_dev(rays), lim_t, tonly, count=True, order=True)),
                           ("numpy", ds.occluded(rays, lim, tonly, count=True, order=True))):
        assert np.array_equal(got, plain) and c == count, (name, what)
    # no limits: nothing but the rays is gathered
    assert np.array_equal(ds.occluded(_dev(rays), None, tonly, order=True), ds.occluded(_dev(rays), None, tonly)), name


def _paths(ds, rays, seeds, tonly, flags=0, **kw):
    return ds.trace_paths(rays, seeds, SCENE, 8, 10, tonly, flags, segments=True, **kw)


def _same_paths(got, want):
    return (tp.differing(got["radiance"], want["radiance"]) == 0 and
            np.array_equal(np.asarray(got["seeds"]).view(np.uint32), np.asarray(want["seeds"]).view(np.uint32)) and
            got["segments"] == want["segments"])


@pytest.mark.parametrize("name", QUERY_SCENES)
def test_trace_paths_through_an_order(name, gpu_available):
    """spp 8, maxBounce 10 with the segment count: ordered equals unordered word for word (tensors and numpy), the first 256
    rays equal the oracle, and two passes [0, 3) with an order and [3, 8) without one equal the one call -- once with
    RTC_F_WAVE_PER_RAY, and once with a precomputed order used by both passes."""
    tris, spheres, tonly, _ = _geometry(name)
    ds = _scene(name)
    rays, seeds, _ = _query_rays(name)
    d, s = _dev(rays), _words(seeds)
    plain = _paths(ds, d, s, bool(tonly))
    assert _same_paths(_paths(ds, d, s, bool(tonly), order=True), plain), (name, "tensor")
    assert _same_paths(_paths(ds, rays, seeds, bool(tonly), order=True), plain), (name, "numpy")
    want = tp.expected(tris, spheres, SCENE, tonly, rays[:256], seeds[:256], 8, 10)
    assert tp.differing(plain["radiance"][:256], want[0]) == 0 and np.array_equal(plain["seeds"][:256], want[1]), name
    import torch

    first = _paths(ds, d, s, bool(tonly), count=3, order=True)
    second = _paths(ds, d, _words(first["seeds"]), bool(tonly), first=3, radiance=torch.from_numpy(first["radiance"]).cuda())
    assert tp.differing(second["radiance"], plain["radiance"]) == 0 and np.array_equal(second["seeds"], plain["seeds"])
    assert first["segments"] + second["segments"] == plain["segments"], name
    first = _paths(ds, d, s, bool(tonly), WAVE, count=3, order=True)
    second = _paths(ds, rays, first["seeds"], bool(tonly), WAVE, first=3, radiance=first["radiance"])
    assert tp.differing(second["radiance"], plain["radiance"]) == 0 and np.array_equal(second["seeds"], plain["seeds"])
    assert first["segments"] + second["segments"] == plain["segments"], (name, "wave")
    order = ds.ray_order(d)
    first = _paths(ds, d, s, bool(tonly), count=3, order=order)
    second = _paths(ds, d, _words(first["seeds"]), bool(tonly), first=3, order=order,
                    radiance=torch.from_numpy(first["radiance"]).cuda())
    assert tp.differing(second["radiance"], plain["radiance"]) == 0 and np.array_equal(second["seeds"], plain["seeds"])
    assert first["segments"] + second["segments"] == plain["segments"], (name, "reused order")


def test_tensor_inputs_use_the_current_stream(gpu_available):
    """On a stream of the caller's, behind work of the caller's on that stream: the tensor path sees the rays that work
    wrote (the order and the query are enqueued there, not on the null stream)."""
    import torch

    ds = _scene("ultracomplex")
    rays = _query_rays("ultracomplex")[0]
    want_order = ds.ray_order(rays)
    want = ds.trace_rays(rays, True)
    side = torch.cuda.Stream()
    staged = _dev(rays)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d = torch.zeros_like(staged)
        for _ in range(20):  # (work on the side stream the copy below has to wait for)
            d.add_(1.0)
        d.copy_(staged)
        order = ds.ray_order(d)
        got = ds.trace_rays(d, True, order=order)
    assert np.array_equal(order.cpu().numpy().view(np.uint32), want_order)
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
