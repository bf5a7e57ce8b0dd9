"""raytracingc_amd -- MI355X-native render path of Atsuyo64/RayTracingC.

The product is librtc.so (HIP kernels for gfx950 behind the C ABI in include/rtc.h).  This package is the
thin host mirror of the reference's interface for that path, with the reference's names:

  scene build   loadOBJTriangles (raytracing.c:100), parseTriangleFile (raytracing.c:76),
                DEFAULT_SPHERES (scene.h:17-19), default_scene (main.c:14,21-28), camera_basis (main.c:252-255)
  render seam   render (main.c:263-304 -> one rtc_render call), render_multi (one process, many GPUs),
                DeviceScene.render_rows_async (device-resident, used by the multi-rank host and bench.py)
  output        vec3ToColor (raytracing.c:11), write_bmp (stbi_write_bmp, main.c:305)
  device probes rayTriangle, raySphere, getEnvironmentLight, RandomValue / RandomValueNormalDistrubtion /
                RandomDiretion -- the renderer's own device functions run on the GPU, for known-answer tests.

There is no CPU fallback: every render call goes to the GPU and raises if librtc.so or the GPU is missing.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._abi import (  # noqa: F401
    CLI_PATH,
    LIB_PATH,
    RAY_DT,
    RTC_F_DEBUG_BOUNCES,
    RTC_F_HOIST_PRIMARY,
    RTC_F_NO_CLUSTER_CULL,
    RTC_F_NO_COOP,
    RTC_F_CHAIN_INLINE,
    RTC_F_OVERLAP,
    RTC_F_HOST_ROWS,
    RTC_F_SPLIT_SPHERES,
    RTC_F_NO_DRAW_CACHE,
    RTC_F_NO_REORDER,
    RTC_F_NO_TILE_CULL,
    RTC_F_WAVE_PER_RAY,
    RTC_DN_DEMODULATE,
    RTC_SEGMENT_COUNTERS,
    RTC_EBUSY,
    RTC_EINVAL,
    RTC_ETIMEDOUT,
    SCENE_DT,
    SPHERE_DT,
    TRIANGLE_DT,
    VEC3_DT,
    EXPORTS,
    Ray,
    RtcCamera,
    RtcChainReport,
    RtcDenoiseDesc,
    RtcError,
    RtcHitBuffers,
    RtcLoopStats,
    RtcPathDesc,
    RtcRenderDesc,
    RtcSampleRange,
    RtcSelectDesc,
    RtcStats,
    Scene,
    Vec3,
    check,
    lib,
)
from ._abi import _ptr

__all__ = [
    "loadOBJTriangles", "parseTriangleFile", "default_spheres", "default_scene", "camera_basis", "RenderConfig",
    "render", "render_multi", "DeviceScene", "vec3ToColor", "write_bmp", "rayTriangle", "raySphere",
    "getEnvironmentLight", "random_sequences", "device_count", "lib", "TRIANGLE_DT", "SPHERE_DT", "RAY_DT",
    "SCENE_DT", "RtcError", "ProgressState", "save_progress", "load_progress", "scene_records_host", "RECORD_ARRAYS",
    "ray_keys_host", "ray_order_scratch_bytes", "gather_async", "scatter_async",
    "regroup_membership_host", "regroup_max_tris", "adaptive_selection",
    "select_desc", "select_pixels", "select_pixels_async", "select_scratch_bytes", "resolve", "resolve_async",
    "denoise_desc", "denoise_scratch_bytes", "denoise_async", "denoise",
]

# main.c:114-116 (camera) and main.c:10-12 (frame) defaults
DEFAULT_ORIGIN = (-4.75, -1.5, -4.75)
DEFAULT_LOOKING_AT = (0.9, -1.2, 1.0)
DEFAULT_FOV = 1.0
DEFAULT_SUN = (-30.0, -85.0, 100.0)


def _take_tris(p: C.c_void_p, n: int) -> np.ndarray:
    out = np.empty(n, dtype=TRIANGLE_DT)
    if n:
        C.memmove(out.ctypes.data, p.value, n * TRIANGLE_DT.itemsize)
    lib().rtc_free(p)
    return out


def loadOBJTriangles(path: str) -> np.ndarray:
    """raytracing.c:100-147 (+ objloader.c): OBJ/MTL -> Triangle[] (x, y negated).  Raises on failure
    (the reference exits 42)."""
    p, n = C.c_void_p(), C.c_int()
    check(lib().rtc_load_obj(path.encode(), C.byref(p), C.byref(n)), "rtc_load_obj")
    return _take_tris(p, n.value)


def parseTriangleFile(path: str) -> np.ndarray:
    """raytracing.c:76-98: triangles.txt -> Triangle[] with counter-clockwise normals."""
    p, n = C.c_void_p(), C.c_int()
    check(lib().rtc_parse_triangle_file(path.encode(), C.byref(p), C.byref(n)), "rtc_parse_triangle_file")
    return _take_tris(p, n.value)


def default_spheres() -> np.ndarray:
    """scene.h:17-19: the single default-mode sphere."""
    p, n = C.c_void_p(), C.c_int()
    check(lib().rtc_default_spheres(C.byref(p), C.byref(n)), "rtc_default_spheres")
    out = np.empty(n.value, dtype=SPHERE_DT)
    C.memmove(out.ctypes.data, p.value, n.value * SPHERE_DT.itemsize)
    return out


def default_scene(sun=DEFAULT_SUN, ground=None, horizon=None, zenith=None, focus=None, intensity=None) -> Scene:
    """main.c:14,21-28 with the CLI overrides of main.c:185-224; the sun is normalised as main.c:247."""
    s = Scene()
    check(lib().rtc_default_scene(C.byref(s)), "rtc_default_scene")
    if ground is not None:
        s.groundColor = Vec3(*ground)
    if horizon is not None:
        s.skyColorHorizon = Vec3(*horizon)
    if zenith is not None:
        s.skyColorZenith = Vec3(*zenith)
    if focus is not None:
        s.sunFocus = focus
    if intensity is not None:
        s.sunIntensity = intensity
    check(lib().rtc_scene_set_sun(C.byref(s), Vec3(*sun)), "rtc_scene_set_sun")
    return s


def camera_basis(origin=DEFAULT_ORIGIN, looking_at=DEFAULT_LOOKING_AT, fov=DEFAULT_FOV) -> RtcCamera:
    """main.c:252-255."""
    cam = RtcCamera()
    check(lib().rtc_camera_basis(Vec3(*origin), Vec3(*looking_at), C.c_float(fov), C.byref(cam)), "rtc_camera_basis")
    return cam


@dataclass
class RenderConfig:
    width: int = 128
    height: int = 128
    spp: int = 4000  # scene.h:26
    max_bounce: int = 10  # main.c:12
    triangles_only: bool = True
    hoist: bool = False
    row_start: int = 0
    row_stride: int = 1
    # rows per interleaved band (rtc.h rowBand): 0/1 single rows y = row_start + k*row_stride; B > 1 (a power of two)
    # bands of B rows starting at row_start + k*row_stride*B
    row_band: int = 0
    debug_bounces: bool = False  # calcDebugColor (raytracing.c:242-260) instead of calcColor
    tile_cull: bool = True  # primary segments visit their 8x8 tile's candidate triangles (bit-exact)
    reorder: bool = True  # dispatch the workgroups that see geometry first (same frame)
    coop: bool = True  # pixels that see geometry: the split launch's rtc_render_chain (same frame)
    cluster_cull: bool = True  # bounce rays skip triangle clusters they provably miss (same frame)
    chain_inline: bool = False  # rtc_render_chain sums each pixel's samples itself (no deferred pass)
    # render_multi: every device copies its rows straight into the host frame instead of the RCCL gather to
    # device 0 (RTC_F_HOST_ROWS; same frame)
    host_rows: bool = False
    # frame pipelining (DeviceScene.render_rows_async): the launch does not join its sky pass into the stream;
    # the frame is complete at the scene's frame event (DeviceScene.set_frame_event); same frame
    overlap: bool = False
    # a launch that renders spheres takes the split launch (tile cull with sphere coverage, sky pass, rtc_render_chain with
    # spheres) whatever the scene's gate decided (DeviceScene.sphere_split; RTC_F_SPLIT_SPHERES; same frame)
    split_spheres: bool = False
    # the launch may read and fill the scene's draw cache (DeviceScene.set_draw_cache); False: RTC_F_NO_DRAW_CACHE, every
    # hit draw computed in the geometry kernel (A/B timing and tests; same frame)
    draw_cache: bool = True

    def flags(self) -> int:
        return ((RTC_F_HOIST_PRIMARY if self.hoist else 0) | (RTC_F_DEBUG_BOUNCES if self.debug_bounces else 0)
                | (0 if self.tile_cull else RTC_F_NO_TILE_CULL) | (0 if self.reorder else RTC_F_NO_REORDER)
                | (0 if self.coop else RTC_F_NO_COOP) | (0 if self.cluster_cull else RTC_F_NO_CLUSTER_CULL)
                | (RTC_F_CHAIN_INLINE if self.chain_inline else 0) | (RTC_F_OVERLAP if self.overlap else 0)
                | (RTC_F_HOST_ROWS if self.host_rows else 0) | (RTC_F_SPLIT_SPHERES if self.split_spheres else 0)
                | (0 if self.draw_cache else RTC_F_NO_DRAW_CACHE))

    def desc(self) -> RtcRenderDesc:
        return RtcRenderDesc(self.width, self.height, self.spp, self.max_bounce, int(self.triangles_only),
                             self.row_start, self.row_stride, self.flags(), self.row_band)

    def rows(self) -> int:
        d = self.desc()
        return lib().rtc_rows_selected(C.byref(d))


def _arr(a, dt):
    if a is None or len(a) == 0:
        return None, 0
    a = np.ascontiguousarray(a, dtype=dt)
    return a, len(a)


def _stats(st: RtcStats) -> dict:
    return {"render_ms": st.renderMs, "frame_ms": st.frameMs, "total_ms": st.totalMs, "segments": st.segments,
            "samples": st.samples, "tri_tests": st.triTests, "cluster_tests": st.clusterTests,
            "discarded_tests": st.discardedTests}


def _vp(p):
    """An address (int; 0 or None: null) as the void pointer ctypes passes."""
    return C.c_void_p(p) if p else None


def _query_rays(who: str, rays):
    """The rays of a query (DeviceScene.trace_rays, trace_paths, occluded) as (on_device, rays, n): a torch tensor on a
    device is read in place, any contiguous one of n x 24 bytes; anything else becomes a contiguous numpy array of
    RAY_DT [n], from RAY_DT [n] or float32 [n, 6]."""
    if hasattr(rays, "data_ptr"):
        nbytes = rays.numel() * rays.element_size()
        if not rays.is_cuda or not rays.is_contiguous() or nbytes % RAY_DT.itemsize:
            raise ValueError(f"{who}: rays must be a contiguous device tensor of whole 24-byte Rays")
        return True, rays, nbytes // RAY_DT.itemsize
    a = np.asarray(rays)
    if a.dtype != RAY_DT:
        if a.ndim != 2 or a.shape[1] != 6:
            raise ValueError(f"{who}: rays must be RAY_DT [n] or float32 [n, 6]")
        a = np.ascontiguousarray(a, np.float32).view(RAY_DT).reshape(-1)
    a = np.ascontiguousarray(a.reshape(-1))
    return False, a, len(a)


@contextlib.contextmanager
def _stream_of(device):
    """`device` made torch's current one: yields its current stream there (the torch stream; .cuda_stream is the
    hipStream_t as an int).  Nothing is synchronised."""
    import torch

    with torch.cuda.device(device):
        yield torch.cuda.current_stream()


@contextlib.contextmanager
def _current_stream_of(device):
    """_stream_of(device), yielding the hipStream_t as an int, and that stream synchronised once the block has enqueued
    its work."""
    with _stream_of(device) as st:
        yield st.cuda_stream
        st.synchronize()


def _six_bounds(who: str, bounds):
    """A ray order's `bounds` as float32 [6] (lo, hi), or None for None (the scene's)."""
    if bounds is None:
        return None
    b = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in bounds]), np.float32)
    if b.size != 6:
        raise ValueError(f"{who}: bounds are (lo, hi): six floats")
    return b


def _adaptive_passes(who: str, passes, spp: int, least: int) -> list:
    """An adaptive frame's `passes` as ints: at least `least` (1 or 2) positive counts summing to at most spp."""
    passes = [int(c) for c in passes]
    if len(passes) < least or any(c <= 0 for c in passes) or sum(passes) > spp:
        raise ValueError(f"{who}: passes {passes} are not {'two or more ' if least == 2 else ''}positive counts summing "
                         f"to at most spp = {spp}")
    return passes


def _host_order(who: str, order, n: int) -> np.ndarray:
    """A caller's precomputed order as host indices [n] (every value below n: numpy's indexing would refuse others).  That
    it is a permutation is not checked: the scatters start from zeros, so a repeated index costs values, not safety."""
    if hasattr(order, "data_ptr"):
        order = order.detach().cpu().numpy()
    idx = np.ascontiguousarray(np.asarray(order).reshape(-1)).astype(np.intp)
    if len(idx) != n or (n and (idx.min() < 0 or idx.max() >= n)):
        raise ValueError(f"{who}: order must hold {n} indices below {n}")
    return idx


def _device_order(who: str, order, n: int, device):
    """A caller's precomputed order as a contiguous int32 tensor [n] on `device`, every value below n (the permutation
    kernels index device memory with it, so it is checked here: one reduction and a host read)."""
    import torch

    if not hasattr(order, "data_ptr"):
        order = torch.from_numpy(_host_order(who, order, n).astype(np.int32))
    order = order.reshape(-1).to(device=device, dtype=torch.int32).contiguous()
    if order.numel() != n or (n and (int(order.min()) < 0 or int(order.max()) >= n)):
        raise ValueError(f"{who}: order must hold {n} indices below {n}")
    return order


def _permuted(scatter: bool, src, order, n: int, elem_bytes: int, stream):
    """A new tensor like `src` (contiguous, on the device, n elements of elem_bytes) holding src[order] (gather), or with
    src[i] at order[i] (scatter), enqueued on `stream`.  A scatter's destination starts zeroed: an order that is no
    permutation leaves zeros, not stale memory, in the elements it never names."""
    import torch

    dst = torch.zeros_like(src) if scatter else torch.empty_like(src)
    if n:
        (scatter_async if scatter else gather_async)(dst.data_ptr(), src.data_ptr(), order.data_ptr(), n, elem_bytes,
                                                     stream)
    return dst


RECORD_ARRAYS = ("tris", "mats", "spheres", "clTris", "clusters", "chunks")  # 64, 32, 48, 64, 32, 32 bytes per record
_RECORD_WORDS = (16, 8, 12, 16, 8, 8)


def _records(call, where: str) -> dict:
    """The six record arrays of rtc_scene_records_host / rtc_probe_scene_records as uint32 [records, dwords]: first the
    sizes (null buffers), then the bytes."""
    sizes = (C.c_size_t * 6)()
    check(call([None] * 6, sizes), where)
    out = [np.zeros((sizes[k] // (4 * w), w), np.uint32) for k, w in enumerate(_RECORD_WORDS)]
    check(call([_ptr(a) for a in out], sizes), where)
    return dict(zip(RECORD_ARRAYS, out))


def scene_records_host(tris, new_tris=None, spheres=None) -> dict:
    """The scene records on the host, no GPU (rtc_scene_records_host): `tris` clustered as an upload clusters them and,
    with new_tris (as many), that grouping refitted to them -- what DeviceScene(tris, spheres) followed by
    update(new_tris) must hold, byte for byte.  Arrays of uint32 dwords by name (RECORD_ARRAYS): in clTris dword 12 is
    the reference index (int32, -1 for padding) and dword 13 the aligned-normal flag; a ball is centre, radius, alpha,
    beta, gamma E, E (float32 bits)."""
    t, nt = _arr(tris, TRIANGLE_DT)
    s, ns = _arr(spheres, SPHERE_DT)
    n, nn = _arr(new_tris, TRIANGLE_DT)
    if n is not None and nn != nt:
        raise ValueError("scene_records_host: new_tris must hold as many triangles as tris")
    return _records(lambda bufs, sizes: lib().rtc_scene_records_host(_ptr(t), nt, _ptr(n), _ptr(s), ns, *bufs, sizes),
                    "rtc_scene_records_host")


def regroup_membership_host(tris) -> np.ndarray:
    """The cluster membership a regroup leaves (rtc_regroup_membership_host), no GPU: int32 [n], the index in `tris` of
    every clustered record.  The device's level-by-level rank count run in plain C++; equal to the upload's membership,
    scene_records_host(tris)["clTris"][:n, 12]."""
    t, nt = _arr(tris, TRIANGLE_DT)
    idx = np.zeros(nt, np.int32)
    check(lib().rtc_regroup_membership_host(_ptr(t), nt, _ptr(idx)), "rtc_regroup_membership_host")
    return idx


def regroup_max_tris() -> int:
    """rtc_scene_regroup_max_tris: the most triangles a regroup takes (above it: upload again)."""
    return int(lib().rtc_scene_regroup_max_tris())


def render(tris, spheres, scene: Scene, cam: RtcCamera, cfg: RenderConfig, device: int = -1,
           want_accum: bool = False):
    """The render seam (main.c:263-304) on one GPU.  Returns (colors uint8 [rows, W, 3],
    accum float32 [rows, W, 3] or None, stats dict)."""
    t, nt = _arr(tris, TRIANGLE_DT)
    s, ns = _arr(spheres, SPHERE_DT)
    rows = cfg.rows()
    colors = np.zeros((rows, cfg.width, 3), np.uint8)
    accum = np.zeros((rows, cfg.width, 3), np.float32) if want_accum else None
    st = RtcStats()
    d = cfg.desc()
    check(lib().rtc_render(_ptr(t), nt, _ptr(s), ns, C.byref(scene), C.byref(cam), C.byref(d), device,
                           _ptr(colors), _ptr(accum), C.byref(st)), "rtc_render")
    return colors, accum, _stats(st)


def render_multi(tris, spheres, scene: Scene, cam: RtcCamera, cfg: RenderConfig, num_devices: int,
                 want_accum: bool = False):
    """Full frame, rows interleaved over `num_devices` GPUs of this process (main.c:84 lifted to GPUs)."""
    t, nt = _arr(tris, TRIANGLE_DT)
    s, ns = _arr(spheres, SPHERE_DT)
    colors = np.zeros((cfg.height, cfg.width, 3), np.uint8)
    accum = np.zeros((cfg.height, cfg.width, 3), np.float32) if want_accum else None
    st = RtcStats()
    d = cfg.desc()
    check(lib().rtc_render_multi(_ptr(t), nt, _ptr(s), ns, C.byref(scene), C.byref(cam), C.byref(d), num_devices,
                                 _ptr(colors), _ptr(accum), C.byref(st)), "rtc_render_multi")
    return colors, accum, _stats(st)


def last_multi_info() -> dict:
    """What this thread's last render_multi ran on (rtc_last_multi_info): path ("none" | "rccl" | "host_rows"), devices,
    and per communicator the rank count RCCL itself reports (ncclCommCount)."""
    path, devs = C.c_int(), C.c_int()
    ranks = (C.c_int * 64)()
    n = lib().rtc_last_multi_info(C.byref(path), C.byref(devs), ranks, 64)
    return {"path": {0: "none", 1: "rccl", 2: "host_rows"}.get(path.value, str(path.value)), "devices": devs.value,
            "comm_ranks": [int(ranks[i]) for i in range(min(n, 64))]}


class DeviceScene:
    """A scene resident in HBM on one device (rtc_scene_upload).  render_rows_async takes raw device
    pointers and a hipStream_t (ints), e.g. from torch tensors / torch.cuda streams."""

    def __init__(self, tris, spheres, device: int = -1):
        t, nt = _arr(tris, TRIANGLE_DT)
        s, ns = _arr(spheres, SPHERE_DT)
        h = C.c_void_p()
        check(lib().rtc_scene_upload(_ptr(t), nt, _ptr(s), ns, device, C.byref(h)), "rtc_scene_upload")
        self._h = h
        self._device = device
        self.tri_count = nt
        self.sphere_count = ns

    def render_rows_async(self, scene: Scene, cam: RtcCamera, cfg: RenderConfig, colors_ptr: int,
                          accum_ptr: int | None = None, segments_ptr: int | None = None, stream: int | None = None):
        d = cfg.desc()
        check(lib().rtc_render_rows_async(self._h, C.byref(scene), C.byref(cam), C.byref(d), C.c_void_p(colors_ptr),
                                          C.c_void_p(accum_ptr) if accum_ptr else None,
                                          C.c_void_p(segments_ptr) if segments_ptr else None,
                                          C.c_void_p(stream) if stream else None), "rtc_render_rows_async")

    def render_samples_async(self, scene: Scene, cam: RtcCamera, cfg: RenderConfig, first: int, count: int,
                             colors_ptr: int, accum_ptr: int, rng_ptr: int, segments_ptr: int | None = None,
                             stream: int | None = None):
        """rtc_render_samples_async: samples [first, first + count) of cfg.spp for every selected pixel, from and into the
        accumulator (float32 [rows, W, 3]) and the RNG states (uint32 [rows, W]) -- a pass of a progressive frame.  Both
        are required; with first == 0 neither is read.  After passes covering [0, spp) in order the buffers and the Color
        frame are those of one launch of spp samples, bit for bit.  Scene, camera, cfg and buffers stay the same across a
        frame's passes, which are ordered on one stream; cfg.overlap is refused."""
        d = cfg.desc()
        rg = RtcSampleRange(int(first), int(count))
        check(lib().rtc_render_samples_async(self._h, C.byref(scene), C.byref(cam), C.byref(d), C.byref(rg),
                                             C.c_void_p(colors_ptr) if colors_ptr else None,
                                             C.c_void_p(accum_ptr) if accum_ptr else None,
                                             C.c_void_p(rng_ptr) if rng_ptr else None,
                                             C.c_void_p(segments_ptr) if segments_ptr else None,
                                             C.c_void_p(stream) if stream else None), "rtc_render_samples_async")

    def render_first_hit_async(self, cam: RtcCamera, cfg: RenderConfig, prim_ptr: int = 0, depth_ptr: int = 0,
                               normal_ptr: int = 0, albedo_ptr: int = 0, stream: int | None = None):
        """rtc_render_first_hit_async: what every selected pixel's primary ray sees (calculateRayCollision,
        raytracing.c:216-240), into the device buffers given (0: not wanted; at least one): prim int32 [rows, W]
        (triangle t >= 0, sphere i as -2 - i, miss -1), depth float32 [rows, W] (999999 on a miss), normal and albedo
        float32 [rows, W, 3] (+0 on a miss), the reference's values bit for bit.  Of cfg only the geometry, the row
        selection, triangles_only and tile_cull count (no scene, samples or bounces).  Asynchronous on `stream`, complete
        there; it leaves the frame and geometry events armed."""
        d = cfg.desc()
        d.flags = 0 if cfg.tile_cull else RTC_F_NO_TILE_CULL
        out = RtcHitBuffers(prim_ptr or None, depth_ptr or None, normal_ptr or None, albedo_ptr or None)
        check(lib().rtc_render_first_hit_async(self._h, C.byref(cam), C.byref(d), C.byref(out),
                                               C.c_void_p(stream) if stream else None), "rtc_render_first_hit_async")

    def first_hit(self, cam: RtcCamera, cfg: RenderConfig, want=("prim", "depth", "normal", "albedo")) -> dict:
        """The first-hit buffers named in `want` as host arrays: allocates torch tensors on the scene's device, launches
        render_first_hit_async on torch's current stream there, synchronises and returns {name: numpy array} -- prim
        int32 [rows, W], depth float32 [rows, W], normal and albedo float32 [rows, W, 3]."""
        import torch

        shapes = {"prim": ((), torch.int32), "depth": ((), torch.float32), "normal": ((3,), torch.float32),
                  "albedo": ((3,), torch.float32)}
        want = tuple(want)
        if not want or any(k not in shapes for k in want):
            raise ValueError(f"DeviceScene.first_hit: want {want!r} is not a non-empty subset of {tuple(shapes)}")
        rows = cfg.rows()
        dev = torch.device("cuda", self._device if self._device >= 0 else torch.cuda.current_device())
        bufs = {k: torch.zeros((rows, cfg.width) + shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
        if rows == 0:  # (nothing selected: the empty tensors have no address to hand over)
            return {k: bufs[k].cpu().numpy() for k in want}
        with _current_stream_of(dev) as st:
            self.render_first_hit_async(cam, cfg, *(bufs[k].data_ptr() if k in bufs else 0 for k in shapes), stream=st)
        return {k: bufs[k].cpu().numpy() for k in want}

    def trace_rays_async(self, rays_ptr: int, n: int, triangles_only: bool = False, flags: int = 0, prim_ptr: int = 0,
                         depth_ptr: int = 0, normal_ptr: int = 0, albedo_ptr: int = 0, stream: int | None = None):
        """rtc_trace_rays_async: the closest hit of n caller-supplied Rays (24 B each: pos, dir; device memory at
        rays_ptr) against the resident scene, calculateRayCollision(ray, trianglesOnly) (raytracing.c:216-240) bit for
        bit, into the device buffers given (0: not wanted; at least one): prim int32 [n] (triangle t >= 0, sphere i as
        -2 - i, miss -1), depth float32 [n] (999999 on a miss), normal and albedo float32 [n, 3] (+0 on a miss).  The
        direction is used as given (not normalised).  flags: 0 or RTC_F_NO_CLUSTER_CULL (every record, the same
        buffers).  Asynchronous on `stream`, complete there; the scene's ordering state and events stay as they were."""
        out = RtcHitBuffers(prim_ptr or None, depth_ptr or None, normal_ptr or None, albedo_ptr or None)
        check(lib().rtc_trace_rays_async(self._h, _vp(rays_ptr), n, int(bool(triangles_only)), flags, C.byref(out),
                                         _vp(stream)), "rtc_trace_rays_async")

    def trace_rays(self, rays, triangles_only: bool = False, want=("prim", "depth", "normal", "albedo"),
                   flags: int = 0, order=None) -> dict:
        """The closest hits of `rays` as host arrays, {name: numpy array} for the names in `want`: prim int32 [n], depth
        float32 [n], normal and albedo float32 [n, 3] (trace_rays_async's values).  `rays`: a numpy array of RAY_DT [n]
        or float32 [n, 6] (pos, dir), which takes the synchronous host entry rtc_trace_rays; or a torch tensor on the
        scene's device (float32 [n, 6], or any contiguous tensor of n x 24 bytes), which is read in place by
        rtc_trace_rays_async on torch's current stream there -- the results are numpy arrays in both cases.
        `order`: None, the rays are traced in the order given, 64 consecutive rays a wave; True, they are
        first put in the coherent order of ray_order (the same values, element for element: the rays are gathered, traced
        and the results scattered back); or a precomputed order (ray_order's, an array or tensor of n indices below n, checked
        here).  It is meant to be a permutation: with repeated indices the elements no index names come back as zeros and
        those named twice hold either result."""
        shapes = {"prim": ((), np.int32), "depth": ((), np.float32), "normal": ((3,), np.float32),
                  "albedo": ((3,), np.float32)}
        want = tuple(want)
        if not want or any(k not in shapes for k in want):
            raise ValueError(f"DeviceScene.trace_rays: want {want!r} is not a non-empty subset of {tuple(shapes)}")
        on_device, a, n = _query_rays("DeviceScene.trace_rays", rays)
        if on_device:
            import torch

            kinds = {np.int32: torch.int32, np.float32: torch.float32}
            bufs = {k: torch.zeros((n,) + shapes[k][0], dtype=kinds[shapes[k][1]], device=rays.device) for k in want}
            if n:
                perm = self._order_for("DeviceScene.trace_rays", order, rays, n)
                with _current_stream_of(rays.device) as st:
                    src = rays if perm is None else _permuted(False, rays, perm, n, 24, st)
                    self.trace_rays_async(src.data_ptr(), n, triangles_only, flags,
                                          *(bufs[k].data_ptr() if k in bufs else 0 for k in shapes), stream=st)
                    if perm is not None:
                        bufs = {k: _permuted(True, b, perm, n, b.element_size() * (b.numel() // n), st)
                                for k, b in bufs.items()}
            return {k: bufs[k].cpu().numpy() for k in want}
        out = {k: np.zeros((n,) + shapes[k][0], shapes[k][1]) for k in want}
        if n:
            perm = self._order_for("DeviceScene.trace_rays", order, a, n)
            if perm is not None:
                a = np.ascontiguousarray(a[perm])
            check(lib().rtc_trace_rays(self._h, _ptr(a), n, int(bool(triangles_only)), flags,
                                       *(_ptr(out[k]) if k in out else None for k in shapes)), "rtc_trace_rays")
            if perm is not None:
                for k, got in out.items():
                    out[k] = np.zeros_like(got)
                    out[k][perm] = got
        return out

    def trace_paths_async(self, scene: Scene, rays_ptr: int, seeds_ptr: int, n: int, spp: int, max_bounce: int,
                          radiance_ptr: int, triangles_only: bool = False, flags: int = 0, first: int = 0,
                          count: int | None = None, seeds_out_ptr: int = 0, segments_ptr: int = 0,
                          stream: int | None = None):
        """rtc_trace_paths_async: the radiance along n caller-supplied Rays (device memory at rays_ptr) with the RNG
        seeds at seeds_ptr (uint32 [n]): samples [first, first + count) of spp (count None: the rest) of main.c:95-100
        with the ray given -- acc = acc + calcColor(ray, trianglesOnly, maxBounce, scene) * (float)(1. / spp) -- into
        radiance_ptr (float32 [n, 3]; read first when first > 0), the RNG states into seeds_out_ptr (0: not wanted; may be
        seeds_ptr) and the number of calculateRayCollision calls added to the u64 at segments_ptr (0: not wanted).  The
        samples of one ray are one RNG chain: one lane per ray runs them in turn, or with flags=RTC_F_WAVE_PER_RAY (alone
        or with RTC_F_NO_CLUSTER_CULL) one wave per ray runs 64 candidate samples at a time -- the same values bit for bit,
        meant for few rays with many samples; the choice is the caller's.  Asynchronous on `stream`, complete there; the
        scene's ordering state and events stay as they were."""
        d = RtcPathDesc(int(spp), int(max_bounce), int(bool(triangles_only)), int(flags), int(first),
                        int(spp) - int(first) if count is None else int(count))
        check(lib().rtc_trace_paths_async(self._h, C.byref(scene), _vp(rays_ptr), _vp(seeds_ptr), n, C.byref(d),
                                          _vp(radiance_ptr), _vp(seeds_out_ptr), _vp(segments_ptr), _vp(stream)),
              "rtc_trace_paths_async")

    def trace_paths(self, rays, seeds, scene: Scene, spp: int, max_bounce: int, triangles_only: bool = False,
                    flags: int = 0, first: int = 0, count: int | None = None, radiance=None,
                    segments: bool = False, order=None) -> dict:
        """The radiance along `rays` as host arrays: {"radiance": float32 [n, 3], "seeds": uint32 [n]} (the RNG states
        after the samples) plus "segments": int (the calculateRayCollision calls) when asked for -- trace_paths_async's
        values for samples [first, first + count) of spp (count None: the rest).  With first > 0 `radiance` is the
        accumulator so far and `seeds` the states the previous call returned.  flags: 0, RTC_F_NO_CLUSTER_CULL,
        RTC_F_WAVE_PER_RAY (a wave per ray instead of a lane; the same values) or both.  `rays` and `seeds` (and `radiance`):
        numpy arrays (RAY_DT [n] or float32 [n, 6]; uint32 [n]; float32 [n, 3]), which take the synchronous host entry
        rtc_trace_paths; or torch tensors on the scene's device, read in place by rtc_trace_paths_async on torch's
        current stream there (the inputs are left as they were) -- the results are numpy arrays in both cases.
        `order`: as trace_rays' -- None, True (ray_order of these rays) or a precomputed order, which the passes of one
        accumulation can share since their rays do not change; the rays, the seeds and (first > 0) the radiance are
        gathered, the radiance and the seeds scattered back: the same values element for element, and the same segment
        count (a sum)."""
        count = int(spp) - int(first) if count is None else int(count)
        if first > 0 and radiance is None:
            raise ValueError("DeviceScene.trace_paths: first > 0 continues an accumulation: pass its radiance")
        on_device, a, n = _query_rays("DeviceScene.trace_paths", rays)
        if on_device:
            import torch

            if not hasattr(seeds, "data_ptr") or seeds.device != rays.device or not seeds.is_contiguous() or \
                    seeds.numel() * seeds.element_size() != 4 * n:
                raise ValueError("DeviceScene.trace_paths: seeds must be a contiguous tensor of n 4-byte words on the rays' device")
            if first > 0:
                if not hasattr(radiance, "data_ptr") or radiance.device != rays.device or \
                        radiance.dtype != torch.float32 or radiance.numel() != 3 * n:
                    raise ValueError("DeviceScene.trace_paths: radiance must be a float32 [n, 3] tensor on the rays' device")
                rad = radiance.contiguous().clone().reshape(n, 3)
            else:
                rad = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)
            out = torch.zeros(n, dtype=torch.int32, device=rays.device)
            seg = torch.zeros(1, dtype=torch.int64, device=rays.device)
            if n:
                perm = self._order_for("DeviceScene.trace_paths", order, rays, n)
                with _current_stream_of(rays.device) as st:
                    src, sds = rays, seeds
                    if perm is not None:
                        src, sds = _permuted(False, rays, perm, n, 24, st), _permuted(False, seeds, perm, n, 4, st)
                        if first > 0:
                            rad = _permuted(False, rad, perm, n, 12, st)
                    self.trace_paths_async(scene, src.data_ptr(), sds.data_ptr(), n, spp, max_bounce, rad.data_ptr(),
                                           triangles_only, flags, first, count, out.data_ptr(),
                                           seg.data_ptr() if segments else 0, stream=st)
                    if perm is not None:
                        rad, out = _permuted(True, rad, perm, n, 12, st), _permuted(True, out, perm, n, 4, st)
            res = {"radiance": rad.cpu().numpy(), "seeds": out.cpu().numpy().view(np.uint32)}
            if segments:
                res["segments"] = int(seg.cpu().numpy()[0])
            return res
        sd =np.ascontiguousarray(np.asarray(seeds).reshape(-1), np.uint32)
        if len(sd) != n:
            raise ValueError(f"DeviceScene.trace_paths: {len(sd)} seeds for {n} rays")
        if first > 0:
            rad = np.array(radiance, np.float32, order="C")  # (a copy: the caller's array is left as it was)
            if rad.size != 3 * n:
                raise ValueError("DeviceScene.trace_paths: radiance must be float32 [n, 3]")
            rad = rad.reshape(n, 3)
        else:
            rad = np.zeros((n, 3), np.float32)
        out = np.zeros(n, np.uint32)
        seg = C.c_ulonglong(0)
        if n:
            perm = self._order_for("DeviceScene.trace_paths", order, a, n)
            if perm is not None:
                a, sd, rad = np.ascontiguousarray(a[perm]), np.ascontiguousarray(sd[perm]), np.ascontiguousarray(rad[perm])
            d = RtcPathDesc(int(spp), int(max_bounce), int(bool(triangles_only)), int(flags), int(first), count)
            check(lib().rtc_trace_paths(self._h, C.byref(scene), _ptr(a), _ptr(sd), n, C.byref(d), _ptr(rad), _ptr(out),
                                        C.cast(C.pointer(seg), C.c_void_p) if segments else None), "rtc_trace_paths")
            if perm is not None:
                rad_g, out_g = rad, out
                rad, out = np.zeros_like(rad_g), np.zeros_like(out_g)
                rad[perm], out[perm] = rad_g, out_g
        res = {"radiance": rad, "seeds": out}
        if segments:
            res["segments"] = int(seg.value)
        return res

    def occluded_async(self, rays_ptr: int, n: int, tmax_ptr: int = 0, triangles_only: bool = False, flags: int = 0,
                       occluded_ptr: int = 0, count_ptr: int = 0, stream: int | None = None):
        """rtc_occluded_async: for n caller-supplied Rays (device memory at rays_ptr) and their limits (float32 [n] at
        tmax_ptr, in units of dir; 0: no limit), whether calculateRayCollision(ray, trianglesOnly) hits with
        dst < tMax (strict, on the reference's own dst): one byte per ray, 0 or 1, at occluded_ptr (any alignment; 0: not
        wanted) and / or the number of occluded rays added to the u64 at count_ptr (0: not wanted); at least one.  The
        direction is used as given: line of sight from a to b is pos = a, dir = b - a, tMax = 1.  flags: 0 or
        RTC_F_NO_CLUSTER_CULL (every record; the same answers).  Asynchronous on `stream`, complete there; the scene's ordering state and events stay as they were."""
        check(lib().rtc_occluded_async(self._h, _vp(rays_ptr), _vp(tmax_ptr), n, int(bool(triangles_only)), int(flags),
                                       _vp(occluded_ptr), _vp(count_ptr), _vp(stream)), "rtc_occluded_async")

    def occluded(self, rays, tmax=None, triangles_only: bool = False, flags: int = 0, count: bool = False,
                 order=None):
        """occluded_async's answers as a numpy bool [n], or (bool [n], int) with count=True (the number of occluded rays,
        counted by the kernel).  `rays`: a numpy array of RAY_DT [n] or float32 [n, 6] (pos, dir), which takes the
        synchronous host entry rtc_occluded; or a torch tensor on the scene's device (float32 [n, 6], or any contiguous
        tensor of n x 24 bytes), read in place by rtc_occluded_async on torch's current stream there.  `tmax`: None (no
        limit), a Python float (the same limit for every ray) or an array / tensor of n float32.  `order`: as trace_rays' --
        None, True or a precomputed order; the rays and limits are gathered and the bytes scattered back (the same answers
        element for element; the count is a sum)."""
        who = "DeviceScene.occluded"
        on_device, a, n = _query_rays(who, rays)
        lim = None
        if tmax is not None:
            if hasattr(tmax, "data_ptr"):  # a tensor: beside device rays it is read in place where it can be
                if tmax.numel() != n:
                    raise ValueError(f"{who}: {tmax.numel()} limits for {n} rays")
                lim = tmax.reshape(-1) if on_device else np.ascontiguousarray(tmax.detach().cpu().numpy().reshape(-1),
                                                                              np.float32)
            else:
                t = np.asarray(tmax, np.float32)
                if t.ndim == 0:
                    t = np.full(n, t, np.float32)
                if t.size != n:
                    raise ValueError(f"{who}: {t.size} limits for {n} rays")
                lim = np.ascontiguousarray(t.reshape(-1))
        if n == 0:
            return (np.zeros(0, bool), 0) if count else np.zeros(0, bool)
        if on_device:
            import torch

            perm = self._order_for(who, order, rays, n)
            with _current_stream_of(rays.device) as st:
                if lim is not None:
                    if isinstance(lim, np.ndarray):
                        lim = torch.from_numpy(lim.copy())  # (a copy: the caller's array may be read-only)
                    lim = lim.to(device=rays.device, dtype=torch.float32).contiguous()
                occ = torch.zeros(n, dtype=torch.uint8, device=rays.device)
                cnt = torch.zeros(1, dtype=torch.int64, device=rays.device)
                src = rays
                if perm is not None:
                    src = _permuted(False, rays, perm, n, 24, st)
                    lim = _permuted(False, lim, perm, n, 4, st) if lim is not None else None
                self.occluded_async(src.data_ptr(), n, lim.data_ptr() if lim is not None else 0, triangles_only, flags,
                                    occ.data_ptr(), cnt.data_ptr() if count else 0, stream=st)
                if perm is not None:
                    occ = _permuted(True, occ, perm, n, 1, st)
            res = occ.cpu().numpy().astype(bool)
            return (res, int(cnt.cpu().numpy()[0])) if count else res
        occ = np.zeros(n, np.uint8)
        cnt = C.c_ulonglong(0)
        perm = self._order_for(who, order, a, n)
        if perm is not None:
            a, lim = np.ascontiguousarray(a[perm]), None if lim is None else np.ascontiguousarray(lim[perm])
        check(lib().rtc_occluded(self._h, _ptr(a), _ptr(lim), n, int(bool(triangles_only)), int(flags), _ptr(occ),
                                 C.cast(C.pointer(cnt), C.c_void_p) if count else None), "rtc_occluded")
        if perm is not None:
            occ_g, occ = occ, np.zeros_like(occ)
            occ[perm] = occ_g
        return (occ.astype(bool), int(cnt.value)) if count else occ.astype(bool)

    def bounds(self):
        """rtc_scene_bounds: (lo, hi), float32 [3] each -- the box of the upload's triangle vertices and sphere extents
        (centre -+ r), the default bounds of the ray order's key.  An update does not move it."""
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        check(lib().rtc_scene_bounds(self._h, _ptr(lo), _ptr(hi)), "rtc_scene_bounds")
        return lo, hi

    def ray_order_async(self, rays_ptr: int, n: int, order_ptr: int, scratch_ptr: int, scratch_bytes: int, bounds=None,
                        keys_ptr: int = 0, stream: int | None = None):
        """rtc_ray_order_async: the stable order of n Rays (device memory at rays_ptr) by their coherence key (DESIGN
        3.15) into order_ptr (uint32 [n]: the permutation that sorts the rays by key, equal keys in ascending index) and,
        where wanted, the keys in input order into keys_ptr (uint32 [n]).  scratch_ptr: ray_order_scratch_bytes(n) bytes
        of device memory, 16-byte aligned.  bounds: None (the scene's, bounds()) or (lo, hi) / six floats, on the host.
        Asynchronous on `stream`, complete there; nothing of the scene's state is touched."""
        b = _six_bounds("DeviceScene.ray_order_async", bounds)
        check(lib().rtc_ray_order_async(self._h, _vp(rays_ptr), n, _ptr(b), _vp(order_ptr), _vp(keys_ptr),
                                        _vp(scratch_ptr), scratch_bytes, _vp(stream)), "rtc_ray_order_async")

    def ray_order(self, rays, bounds=None, keys: bool = False):
        """The coherent order of `rays` (ray_order_async's): the permutation that sorts them by key, stably -- equal to
        np.argsort(ray_keys_host(rays, lo, hi), kind="stable") -- or (order, keys) with keys=True.  numpy rays (RAY_DT [n]
        or float32 [n, 6]) take the synchronous host entry rtc_ray_order and give numpy uint32 arrays; a torch tensor on
        the scene's device is sorted in place of residence on torch's current stream there and gives int32 tensors on that
        device.  Pass the result as `order=` to trace_rays, trace_paths or occluded."""
        on_device, a, n = _query_rays("DeviceScene.ray_order", rays)
        b = _six_bounds("DeviceScene.ray_order", bounds)
        if on_device:
            import torch

            order = torch.zeros(n, dtype=torch.int32, device=rays.device)
            kt = torch.zeros(n, dtype=torch.int32, device=rays.device) if keys else None
            if n:
                nbytes = ray_order_scratch_bytes(n)
                scratch = _scratch(nbytes, rays.device)
                with _current_stream_of(rays.device) as st:
                    self.ray_order_async(rays.data_ptr(), n, order.data_ptr(), scratch.data_ptr(), nbytes, b,
                                         kt.data_ptr() if keys else 0, stream=st)
            return (order, kt) if keys else order
        order = np.zeros(n, np.uint32)
        ks = np.zeros(n, np.uint32) if keys else None
        if n:
            check(lib().rtc_ray_order(self._h, _ptr(a), n, _ptr(b), _ptr(order), _ptr(ks)), "rtc_ray_order")
        return (order, ks) if keys else order

    def _order_for(self, who: str, order, rays, n: int):
        """A query's `order=` as what its path permutes with: None (no order); for device rays an int32 tensor there, for
        host rays numpy indices.  True computes ray_order(rays)."""
        if order is None or order is False:
            return None
        on_device = hasattr(rays, "data_ptr")
        if order is True:
            got = self.ray_order(rays)
            return got if on_device else got.astype(np.intp)
        return _device_order(who, order, n, rays.device) if on_device else _host_order(who, order, n)

    def render_progressive(self, scene: Scene, cam: RtcCamera, cfg: RenderConfig, passes, state: "ProgressState | None" = None):
        """A generator over the passes of one frame: `passes` is a list of sample counts summing to cfg.spp (or, with
        `state` -- a frame saved earlier, load_progress -- to the samples it still lacks).  It owns the three device
        buffers (torch tensors on the current device) and after each pass yields (samples_done, colors uint8 [rows, W, 3],
        accum float32 [rows, W, 3]) as host arrays: the reference's frame after samples_done iterations of main.c:98-99,
        darker than the finished one by samples_done / spp.  self.progress is then the frame's ProgressState (for
        save_progress).  Stop iterating to cancel."""
        import torch

        passes = [int(c) for c in passes]
        done = state.samples_done if state is not None else 0
        if state is not None:
            state.check(cfg)
        if any(c <= 0 for c in passes) or done + sum(passes) != cfg.spp:
            raise ValueError(f"render_progressive: passes {passes} after {done} samples do not sum to spp = {cfg.spp}")
        rows = cfg.rows()
        colors = torch.zeros((rows, cfg.width, 3), dtype=torch.uint8, device="cuda")
        if state is not None:
            accum = torch.from_numpy(np.ascontiguousarray(state.accum, np.float32)).cuda()
            rng = torch.from_numpy(np.ascontiguousarray(state.rng, np.uint32).view(np.int32)).cuda()
        else:
            accum = torch.zeros((rows, cfg.width, 3), dtype=torch.float32, device="cuda")
            rng = torch.zeros((rows, cfg.width), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        for count in passes:
            self.render_samples_async(scene, cam, cfg, done, count, colors.data_ptr(), accum.data_ptr(), rng.data_ptr(),
                                      None, st)
            done += count
            torch.cuda.synchronize()
            host_accum = accum.cpu().numpy()
            self.progress = ProgressState(host_accum, rng.cpu().numpy().view(np.uint32), done, ProgressState.fields_of(cfg))
            yield done, colors.cpu().numpy(), host_accum

    def render_pixels_async(self, scene: Scene, cam: RtcCamera, cfg: RenderConfig, first: int, count: int,
                            pixels_ptr: int, n: int, accum_ptr: int, rng_ptr: int, colors_ptr: int = 0,
                            segments_ptr: int | None = None, flags: int = 0, stream: int | None = None):
        """rtc_render_pixels_async: samples [first, first + count) of cfg.spp for the n pixels listed at
        pixels_ptr (uint32 compact indices launch_row * W + x, device memory) of a progressive frame, from and into the
        frame's own buffers -- accum float32 [rows, W, 3], rng uint32 [rows, W], colors uint8 [rows, W, 3] (0: not wanted)
        -- in place: a listed pixel holds what render_samples_async over the same range leaves there, bit for bit, every
        other pixel its bytes as they were; an index >= rows * W is skipped.  With first == 0 neither buffer is read.
        segments_ptr: ONE u64 the launch adds its calculateRayCollision calls to.  flags: 0, RTC_F_NO_CLUSTER_CULL,
        RTC_F_WAVE_PER_RAY (a wave per listed pixel: few pixels with many samples) or both; of cfg's own flags
        debug_bounces and overlap are refused and the rest ignored.  Asynchronous on `stream`, complete there; the scene's
        ordering state and events stay as they were."""
        d = cfg.desc()
        rg = RtcSampleRange(int(first), int(count))
        check(lib().rtc_render_pixels_async(self._h, C.byref(scene), C.byref(cam), C.byref(d), C.byref(rg),
                                            _vp(pixels_ptr), int(n), int(flags), _vp(colors_ptr), _vp(accum_ptr),
                                            _vp(rng_ptr), _vp(segments_ptr), _vp(stream)), "rtc_render_pixels_async")

    def render_pixels(self, scene: Scene, cam: RtcCamera, cfg: RenderConfig, first: int, count: int, pixels, accum, rng,
                      colors=None, segments: bool = False, flags: int = 0) -> dict:
        """A pass over the listed pixels of a progressive frame (render_pixels_async's values): {"accum", "rng"} plus
        "colors" where given and "segments": int when asked for.  `pixels`: compact indices launch_row * W + x.  Either
        everything is numpy -- pixels any integer array, accum float32 [rows, W, 3], rng uint32 [rows, W], colors uint8
        [rows, W, 3] or None -- which takes the synchronous host entry rtc_render_pixels on copies (the caller's arrays are
        left as they were, the results are new arrays); or everything is a contiguous torch tensor on the scene's device
        (pixels and rng any 4-byte integer type), updated in place by rtc_render_pixels_async on torch's current stream
        there: the result holds the same tensors."""
        who = "DeviceScene.render_pixels"
        npix = cfg.rows() * cfg.width
        if hasattr(pixels, "data_ptr"):
            import torch

            dev = pixels.device
            n = pixels.numel()
            sizes = (("pixels", pixels, 4 * n), ("accum", accum, 12 * npix), ("rng", rng, 4 * npix), ("colors", colors, 3 * npix))
            for name, t, nbytes in sizes:
                if t is None and name == "colors":
                    continue
                if not hasattr(t, "data_ptr") or not t.is_cuda or t.device != dev or not t.is_contiguous() or \
                        t.numel() * t.element_size() != nbytes:
                    raise ValueError(f"{who}: {name} must be a contiguous tensor of {nbytes} bytes on the list's device")
            if pixels.element_size() != 4 or rng.element_size() != 4 or accum.dtype != torch.float32:
                raise ValueError(f"{who}: pixels and rng are 4-byte integers, accum is float32")
            seg = torch.zeros(1, dtype=torch.int64, device=dev)
            if n and npix:
                with _current_stream_of(dev) as st:
                    self.render_pixels_async(scene, cam, cfg, first, count, pixels.data_ptr(), n, accum.data_ptr(),
                                             rng.data_ptr(), colors.data_ptr() if colors is not None else 0,
                                             seg.data_ptr() if segments else None, flags, st)
            res = {"accum": accum, "rng": rng}
            if colors is not None:
                res["colors"] = colors
            if segments:
                res["segments"] = int(seg.cpu().numpy()[0])
            return res
        px = np.asarray(pixels).reshape(-1)
        if px.size and (not np.issubdtype(px.dtype, np.integer) or px.min() < 0 or px.max() > 0xffffffff):
            raise ValueError(f"{who}: pixels must be integers in [0, 2^32)")
        px = np.ascontiguousarray(px, np.uint32)
        acc = np.array(accum, np.float32, order="C")  # (copies: the caller's arrays are left as they were)
        state = np.array(rng, np.uint32, order="C")
        col = None if colors is None else np.array(colors, np.uint8, order="C")
        if acc.size != 3 * npix or state.size != npix or (col is not None and col.size != 3 * npix):
            raise ValueError(f"{who}: accum float32 [rows, W, 3], rng uint32 [rows, W] and colors uint8 [rows, W, 3] of "
                             f"the frame's {npix} pixels")
        seg = C.c_ulonglong(0)
        if len(px) and npix:
            d = cfg.desc()
            rg = RtcSampleRange(int(first), int(count))
            check(lib().rtc_render_pixels(self._h, C.byref(scene), C.byref(cam), C.byref(d), C.byref(rg), _ptr(px), len(px),
                                          int(flags), _ptr(col), _ptr(acc), _ptr(state),
                                          C.cast(C.pointer(seg), C.c_void_p) if segments else None), "rtc_render_pixels")
        res = {"accum": acc, "rng": state}
        if col is not None:
            res["colors"] = col
        if segments:
            res["segments"] = int(seg.value)
        return res

    def render_adaptive(self, scene: Scene, cam: RtcCamera, cfg: RenderConfig, passes, select, flags: int = 0):
        """A generator over the passes of one adaptively sampled frame: `passes` is a list of sample counts summing to at
        most cfg.spp.  The first is a whole pass (render_samples_async); every further one is a pass over the pixels that
        `select(done, colors, accum, samples)` returns before it (render_pixels_async with `flags`): compact indices
        launch_row * W + x, which must be a subset of the previous pass's pixels -- all at samples == done, none twice --
        or ValueError is raised; an empty selection ends the frame.  It owns the three device buffers (torch tensors on the
        current device) and after each pass yields (done, colors uint8 [rows, W, 3], accum float32 [rows, W, 3], samples
        int32 [rows, W]) as host arrays: `samples` is what each pixel has had, `done` the most any has; a pixel's sum and
        state are the reference's after its own number of samples, weighted 1 / spp each, so a caller normalises with
        accum * spp / samples.  Stop iterating to cancel."""
        import torch

        passes = _adaptive_passes("render_adaptive", passes, cfg.spp, 1)
        rows = cfg.rows()
        colors = torch.zeros((rows, cfg.width, 3), dtype=torch.uint8, device="cuda")
        accum = torch.zeros((rows, cfg.width, 3), dtype=torch.float32, device="cuda")
        rng = torch.zeros((rows, cfg.width), dtype=torch.int32, device="cuda")
        samples = np.zeros((rows, cfg.width), np.int32)
        st = torch.cuda.current_stream().cuda_stream
        done, host = 0, None
        for k, count in enumerate(passes):
            if k == 0:
                self.render_samples_async(scene, cam, cfg, 0, count, colors.data_ptr(), accum.data_ptr(), rng.data_ptr(),
                                          None, st)
                samples += count
            else:
                sel = adaptive_selection(select(done, host[0], host[1], samples.copy()), samples, done)
                if len(sel) == 0:
                    return
                pixels = torch.from_numpy(sel.view(np.int32)).cuda()
                self.render_pixels_async(scene, cam, cfg, done, count, pixels.data_ptr(), len(sel), accum.data_ptr(),
                                         rng.data_ptr(), colors.data_ptr(), None, flags, st)
                samples.reshape(-1)[sel] += count
            done += count
            torch.cuda.synchronize()
            host = (colors.cpu().numpy(), accum.cpu().numpy())
            yield done, host[0], host[1], samples.copy()

    def render_adaptive_device(self, scene: Scene, cam: RtcCamera, cfg: RenderConfig, passes, threshold: float,
                               floor: float, capacity: int, flags: int = RTC_F_WAVE_PER_RAY) -> dict:
        """One adaptively sampled frame enqueued whole on torch's current stream, without one synchronisation or host read
        (DESIGN 3.20).  `passes`: at least two sample counts summing to at most cfg.spp.  Passes 0 and 1 are whole passes
        (render_samples_async); a snapshot of the accumulator is taken before every pass from 1 on (a device-to-device
        copy), and after it select_pixels_async judges the pixels the pass rendered -- every pixel after pass 1, the last
        list after a later one -- with select_desc(cfg.spp, before, done, threshold, floor) and stamps `done` into
        `samples`; its output, cut at `capacity`, is the list of the next pass (render_pixels_async with n = capacity and
        `flags`; the sentinel tail is skipped there), alternating between two list buffers.  The last pass's select only
        stamps and counts (capacity 0), and resolve_async makes the displayable frame.  Returns device tensors: "colors"
        uint8 [rows, W, 3] (resolved), "accum" float32 [rows, W, 3], "rng" int32 [rows, W], "samples" int32 [rows, W] and
        "counts" int64 [len(passes) - 1]: what each select chose BEFORE the cut at capacity.  Nothing is complete until
        the stream is."""
        import torch

        passes = _adaptive_passes("render_adaptive_device", passes, cfg.spp, 2)
        capacity = int(capacity)
        if not 1 <= capacity <= 0x7fffffff:
            raise ValueError(f"render_adaptive_device: a capacity of {capacity} pixels")
        rows, width = cfg.rows(), cfg.width
        npix = rows * width
        dev = torch.device("cuda", torch.cuda.current_device())
        colors = torch.zeros((rows, width, 3), dtype=torch.uint8, device=dev)
        accum = torch.zeros((rows, width, 3), dtype=torch.float32, device=dev)
        prev = torch.empty_like(accum)
        rng = torch.zeros((rows, width), dtype=torch.int32, device=dev)
        samples = torch.zeros((rows, width), dtype=torch.int32, device=dev)
        counts = torch.zeros(len(passes) - 1, dtype=torch.int64, device=dev)
        lists = [torch.full((capacity,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
        nbytes = select_scratch_bytes(max(npix, capacity))
        scratch = _scratch(nbytes, dev)
        res = {"colors": colors, "accum": accum, "rng": rng, "samples": samples, "counts": counts}
        if npix == 0:
            return res
        st = torch.cuda.current_stream().cuda_stream
        self.render_samples_async(scene, cam, cfg, 0, passes[0], colors.data_ptr(), accum.data_ptr(), rng.data_ptr(), None,
                                  st)
        done, cur = passes[0], None  # cur: the list buffer the next pass renders (None: every pixel)
        for k in range(1, len(passes)):
            before, done = done, done + passes[k]
            prev.copy_(accum)
            if cur is None:
                self.render_samples_async(scene, cam, cfg, before, passes[k], colors.data_ptr(), accum.data_ptr(),
                                          rng.data_ptr(), None, st)
            else:
                self.render_pixels_async(scene, cam, cfg, before, passes[k], lists[cur].data_ptr(), capacity,
                                         accum.data_ptr(), rng.data_ptr(), 0, None, flags, st)
            last = k == len(passes) - 1
            nxt = 0 if cur is None else 1 - cur
            select_pixels_async(accum.data_ptr(), prev.data_ptr(), npix, None if cur is None else lists[cur].data_ptr(),
                                0 if cur is None else capacity, select_desc(cfg.spp, before, done, threshold, floor),
                                None if last else lists[nxt].data_ptr(), 0 if last else capacity,
                                counts.data_ptr() + 8 * (k - 1), samples.data_ptr(), scratch.data_ptr(), nbytes, st)
            cur = nxt
        resolve_async(accum.data_ptr(), samples.data_ptr(), npix, cfg.spp, colors.data_ptr(), st)
        return res

    @property
    def chain_wgs(self) -> int:
        """rtc_render_chain's workgroups per CU for whole frames, chosen at upload (rtc_scene_chain_wgs)."""
        return lib().rtc_scene_chain_wgs(self._h)

    def chain_report(self) -> dict:
        """What the scene's last geometry-kernel launch chose (rtc_scene_chain_report; host state, no device work): the
        kernel's template flags multi, count, hits, general, spheres, resume and chain_prim_f (the primary filter records
        staged in LDS) as bools; wgs_per_cu, chain_dyn (bytes of dynamic LDS), cluster_count, chunk_count and launches
        (the geometry-kernel launches enqueued so far; 0: no launch yet) as ints."""
        r = RtcChainReport()
        check(lib().rtc_scene_chain_report(self._h, C.byref(r)), "rtc_scene_chain_report")
        out = {k: bool(getattr(r, k)) for k in ("multi", "count", "hits", "general", "spheres", "resume")}
        out.update(chain_prim_f=bool(r.chainPrimF), wgs_per_cu=r.wgsPerCu, chain_dyn=r.chainDyn,
                   cluster_count=r.clusterCount, chunk_count=r.chunkCount, launches=r.launches)
        return out

    def last_plan(self):
        """What the scene's most recent enqueue planned (rtc_scene_last_plan; host state, no device work), in the planner
        hooks' encoding: (ops int32 [n, 4]: kind, stream, event, kernel; rows uint64 [m, 6]: op index, res, access, id, lo,
        hi, the trailing ~0 record last).  Before anything was enqueued both are empty."""
        ops = np.zeros((48, 4), np.int32)
        fp = np.zeros((256, 6), np.uint64)
        rc = lib().rtc_scene_last_plan(self._h, _ptr(ops), 48, _ptr(fp), 256)
        if rc < 0:
            raise RtcError(rc, "rtc_scene_last_plan")
        return ops[: rc & 0xff].copy(), fp[: rc >> 8].copy()

    def spans(self):
        """Every device allocation the scene owns (rtc_scene_spans; host state, no device work): uint64 [n, 5] rows of
        res, id, part, base, bytes -- res and id in the footprint rows' numbering, bytes 0 where nothing is allocated yet."""
        out = np.zeros((64, 5), np.uint64)
        rc = lib().rtc_scene_spans(self._h, _ptr(out), 64)
        if rc < 0:
            raise RtcError(rc, "rtc_scene_spans")
        return out[:rc].copy()

    def set_draw_cache(self, blocks: int = -1):
        """The draw cache's capacity in 1-KB blocks, one per cached pixel (rtc_scene_set_draw_cache): 0 disables it, a
        negative value restores the default.  Synchronises the device and drops what is cached."""
        check(lib().rtc_scene_set_draw_cache(self._h, int(blocks)), "rtc_scene_set_draw_cache")

    def draw_cache_reset(self):
        """Forget every cached pixel (rtc_scene_draw_cache_reset; synchronises the device)."""
        check(lib().rtc_scene_draw_cache_reset(self._h), "rtc_scene_draw_cache_reset")

    def draw_cache_stats(self) -> dict:
        """rtc_scene_draw_cache_stats (synchronises the device): blocks in use, capacity (0 before the first launch that
        uses the cache), and the last such launch's fresh (newly cached) and uncached items."""
        out = (C.c_ulonglong * 4)()
        check(lib().rtc_scene_draw_cache_stats(self._h, out), "rtc_scene_draw_cache_stats")
        return {"blocks": int(out[0]), "capacity": int(out[1]), "fresh": int(out[2]), "uncached": int(out[3])}

    def draw_cache_block(self, seed: int):
        """The cached block of the pixel with this seed (x + y * width), float32 [64, 4] -- entry j: RandomDiretion from
        the seed advanced 7 j draws, then the roulette value -- or None when the pixel has none (rtc_probe_draw_cache)."""
        out = np.zeros((64, 4), np.float32)
        blk = C.c_int(-1)
        check(lib().rtc_probe_draw_cache(self._h, int(seed), _ptr(out), C.byref(blk)), "rtc_probe_draw_cache")
        return out if blk.value >= 0 else None

    @property
    def sphere_split(self) -> bool:
        """Whether launches that render this scene's spheres take the split launch by default, decided at upload
        (rtc_scene_sphere_split: at most 32 spheres, at least one triangle and a bounce-hit share, spheres included, of
        at most 0.5)."""
        return bool(lib().rtc_scene_sphere_split(self._h))

    def set_timing(self, enable: bool):
        """Record HIP events around the split launch's kernels from now on (rtc_scene_set_timing)."""
        check(lib().rtc_scene_set_timing(self._h, int(enable)), "rtc_scene_set_timing")

    def set_geometry_event(self, event_handle: int | None):
        """Arm this hipEvent_t (e.g. a torch.cuda.Event's cuda_event) for the NEXT launch only: it records it on its
        stream once the geometry-pixel kernels are enqueued, before the sky pass joins, and forgets it
        (rtc_scene_set_geometry_event, one-shot); None disarms."""
        check(lib().rtc_scene_set_geometry_event(self._h, C.c_void_p(event_handle) if event_handle else None),
              "rtc_scene_set_geometry_event")

    def set_frame_event(self, event_handle: int | None):
        """Arm this hipEvent_t for the NEXT launch only: it records it once its whole frame is written (on its stream
        after the join, or with RenderConfig.overlap on the scene's side stream) and forgets it
        (rtc_scene_set_frame_event, one-shot); None disarms.  A later launch never records it, so releasing the
        event after that launch is safe.  (A torch.cuda.Event has no hipEvent_t before its first record: record
        it once first.)"""
        check(lib().rtc_scene_set_frame_event(self._h, C.c_void_p(event_handle) if event_handle else None),
              "rtc_scene_set_frame_event")

    def frame_loop(self, scene: Scene, cam, cfg: RenderConfig, dev_rows: list, host_rows: list,
                   host_pitch: int, frames: int, stream: int | None = None) -> dict:
        """rtc_frame_loop: `frames` pipelined frames of cfg's rows, rendered into the device buffers dev_rows[k % n]
        and copied (SDMA, native copy thread) into the page-locked host buffers host_rows[k % n] with row pitch
        host_pitch; returns when the last frame is in host memory.  `cam` is one RtcCamera, or a sequence of them:
        frame k then renders with cam[k % len(cam)] (rtc_frame_loop_cameras, a moving camera)."""
        n = len(dev_rows)
        if len(host_rows) != n:
            raise ValueError("frame_loop: one host buffer per device buffer")
        d = cfg.desc()
        dv = (C.c_void_p * n)(*dev_rows)
        hv = (C.c_void_p * n)(*host_rows)
        st = RtcLoopStats()
        strm = C.c_void_p(stream) if stream else None
        if isinstance(cam, RtcCamera):
            check(lib().rtc_frame_loop(self._h, C.byref(scene), C.byref(cam), C.byref(d), dv, hv,
                                       C.c_size_t(host_pitch), n, int(frames), strm, C.byref(st)), "rtc_frame_loop")
        else:
            cams = (RtcCamera * len(cam))(*cam)
            check(lib().rtc_frame_loop_cameras(self._h, C.byref(scene), cams, len(cam), C.byref(d), dv, hv,
                                               C.c_size_t(host_pitch), n, int(frames), strm, C.byref(st)),
                  "rtc_frame_loop_cameras")
        return {"wall_ms": st.wallMs, "frames": st.frames, "enqueue_ms": st.enqueueMs,
                "copy_ms_median": st.copyMsMedian, "copy_ms_max": st.copyMsMax}

    def kernel_times(self):
        """(heavy-tile kernel ms, sky kernel ms) of the last split launch (None if it was not one)."""
        out = (C.c_float * 2)()
        check(lib().rtc_scene_kernel_times(self._h, out), "rtc_scene_kernel_times")
        return None if out[0] < 0 else (float(out[0]), float(out[1]))

    def regroup_scratch_bytes(self) -> int:
        """rtc_scene_regroup_scratch_bytes: the device scratch regroup_async needs for this scene."""
        return int(lib().rtc_scene_regroup_scratch_bytes(self._h))

    def regroup_async(self, tris_ptr: int, spheres_ptr: int | None, scratch_ptr: int, scratch_bytes: int,
                      stream: int | None = None):
        """rtc_scene_regroup_async: an update from the device arrays at tris_ptr (required, the upload's count) and
        spheres_ptr (0 / None: the spheres are kept) that first decides the clusters anew from those triangles, on the
        device; afterwards the scene holds what a fresh upload of them would, byte for byte.  scratch_ptr:
        regroup_scratch_bytes() bytes of device memory, 16-byte aligned.  Asynchronous on `stream`, ordered as an update."""
        if not self._h:
            raise RuntimeError("DeviceScene.regroup_async: the scene has been released")
        check(lib().rtc_scene_regroup_async(self._h, _vp(tris_ptr), self.tri_count, _vp(spheres_ptr),
                                            self.sphere_count if spheres_ptr else 0, _vp(scratch_ptr), scratch_bytes,
                                            _vp(stream)), "rtc_scene_regroup_async")

    def update(self, tris=None, spheres=None, stream: int | None = None, regroup: bool = False):
        """Replace the resident triangles and / or spheres in place (rtc_scene_update / rtc_scene_update_async): the
        counts are the upload's, None leaves that kind unchanged.  Numpy arrays of TRIANGLE_DT / SPHERE_DT take the
        synchronous host path.  Torch tensors on the scene's device (any dtype, count x 68 / 36 bytes, contiguous) take
        the asynchronous path on `stream` (a hipStream_t; None: torch's current stream): every launch enqueued on the
        scene afterwards renders the new geometry, every earlier one the old, and the tensors may be reused once the
        stream has passed the call.  The upload's scheduling hints stay; the frames are the new geometry's bit for bit.
        regroup=True also decides the clusters anew from `tris` (required then) on the device, as a fresh upload of them
        would (rtc_scene_regroup / rtc_scene_regroup_async; at most regroup_max_tris() triangles): the frames are the
        same, the culling is that of a fresh upload.  The device path allocates its scratch on torch's current stream."""
        if not self._h:
            raise RuntimeError("DeviceScene.update: the scene has been released")
        if tris is None and spheres is None:
            raise ValueError("DeviceScene.update: neither triangles nor spheres")
        if regroup and tris is None:
            raise ValueError("DeviceScene.update: regroup=True needs the triangles (the clusters are decided from them)")
        on_device = [hasattr(a, "data_ptr") for a in (tris, spheres) if a is not None]
        if not any(on_device):
            t, nt = _arr(tris, TRIANGLE_DT)
            s, ns = _arr(spheres, SPHERE_DT)
            if regroup:
                check(lib().rtc_scene_regroup(self._h, _ptr(t), nt, _ptr(s), ns), "rtc_scene_regroup")
            else:
                check(lib().rtc_scene_update(self._h, _ptr(t), nt, _ptr(s), ns), "rtc_scene_update")
            return
        if not all(on_device):
            raise TypeError("DeviceScene.update: triangles and spheres both on the host or both on the device")
        import torch

        def dev(a, item, what):
            if a is None:
                return None, 0
            nbytes = a.numel() * a.element_size()
            if not a.is_cuda or not a.is_contiguous() or nbytes % item:
                raise ValueError(f"DeviceScene.update: {what} must be a contiguous device tensor of whole {item}-byte records")
            return C.c_void_p(a.data_ptr()), nbytes // item

        pt, nt = dev(tris, TRIANGLE_DT.itemsize, "tris")
        ps, ns = dev(spheres, SPHERE_DT.itemsize, "spheres")
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        if regroup:
            # (torch's allocator hands the scratch back to its current stream: a caller on another `stream` orders the two)
            nbytes = self.regroup_scratch_bytes()
            scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=tris.device)
            check(lib().rtc_scene_regroup_async(self._h, pt, nt, ps, ns, C.c_void_p(scratch.data_ptr()), nbytes,
                                                C.c_void_p(stream) if stream else None), "rtc_scene_regroup_async")
            if stream != torch.cuda.current_stream(tris.device).cuda_stream:
                scratch.record_stream(torch.cuda.ExternalStream(stream, device=tris.device))
            return
        check(lib().rtc_scene_update_async(self._h, pt, nt, ps, ns, C.c_void_p(stream) if stream else None),
              "rtc_scene_update_async")

    def records(self) -> dict:
        """The records a launch enqueued now would read, copied back after a device synchronisation
        (rtc_probe_scene_records): the arrays of scene_records_host, for the tests of update()."""
        if not self._h:
            raise RuntimeError("DeviceScene.records: the scene has been released")
        return _records(lambda bufs, sizes: lib().rtc_probe_scene_records(self._h, *bufs, sizes), "rtc_probe_scene_records")

    def close(self):
        if self._h:
            lib().rtc_scene_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class ProgressState:
    """A progressive frame between two passes (DeviceScene.render_progressive): per pixel the float accumulator and the RNG
    state -- 16 bytes, all a pass needs to go on --, the samples done, and the RenderConfig fields that decide the
    pixels' values (a frame is continued with the same ones; the scene and the camera are the caller's to keep)."""
    accum: np.ndarray  # float32 [rows, W, 3]
    rng: np.ndarray  # uint32 [rows, W]
    samples_done: int
    cfg: dict

    FIELDS = ("width", "height", "spp", "max_bounce", "triangles_only", "row_start", "row_stride", "row_band",
              "debug_bounces")

    @staticmethod
    def fields_of(cfg: RenderConfig) -> dict:
        return {k: int(getattr(cfg, k)) for k in ProgressState.FIELDS}

    def check(self, cfg: RenderConfig) -> None:
        if self.cfg != ProgressState.fields_of(cfg):
            raise ValueError(f"the saved frame was rendered with {self.cfg}, not {ProgressState.fields_of(cfg)}")
        if self.accum.shape != (cfg.rows(), cfg.width, 3) or self.rng.shape != (cfg.rows(), cfg.width):
            raise ValueError("the saved frame's buffers do not have the launch's shape")
        if not 0 < self.samples_done <= cfg.spp:
            raise ValueError(f"the saved frame has {self.samples_done} of {cfg.spp} samples")


def adaptive_selection(selection, samples, done: int) -> np.ndarray:
    """What DeviceScene.render_adaptive accepts from its `select` callback, as uint32 compact indices in the order given:
    integers below samples.size, none twice, every one a pixel of the previous pass (samples == done there; `samples`:
    int [rows, W], the samples each pixel has had).  Anything else raises ValueError; an empty selection is fine."""
    sel = np.asarray(selection).reshape(-1)
    if sel.size == 0:
        return np.zeros(0, np.uint32)
    flat = np.asarray(samples).reshape(-1)
    if not np.issubdtype(sel.dtype, np.integer):
        raise ValueError("render_adaptive: the selection must be integer pixel indices")
    sel = sel.astype(np.int64)
    if sel.min() < 0 or sel.max() >= flat.size:
        raise ValueError(f"render_adaptive: the selection names a pixel outside the frame's {flat.size}")
    if len(np.unique(sel)) != len(sel):
        raise ValueError("render_adaptive: the selection names a pixel twice")
    if np.any(flat[sel] != done):
        raise ValueError(f"render_adaptive: the selection is not a subset of the previous pass's pixels (every pixel that "
                         f"goes on has had all {done} samples)")
    return np.ascontiguousarray(sel, np.uint32)


def select_desc(spp: int, before: int, done: int, threshold: float, floor: float) -> RtcSelectDesc:
    """The RtcSelectDesc that compares the mean of samples [before, done) of a frame of `spp` with the mean of samples
    [0, before) (include/rtc.h): wAccum = spp / (done - before), wPrev = wAccum + spp / before and wLevel =
    spp / done, computed in double and rounded once to f32; samplesDone = done."""
    spp, before, done = int(spp), int(before), int(done)
    if not 0 < before < done or spp <= 0:
        raise ValueError(f"select_desc: 0 < before < done and spp > 0, not before = {before}, done = {done}, spp = {spp}")
    w_accum = spp / (done - before)
    return RtcSelectDesc(w_accum, w_accum + spp / before, spp / done, float(floor), float(threshold), done)


def select_scratch_bytes(n: int) -> int:
    """rtc_select_scratch_bytes: the device scratch rtc_select_pixels_async needs for an input sequence of n entries (the
    list's length, or the pixel count without a list)."""
    return int(lib().rtc_select_scratch_bytes(int(n)))


def select_pixels_async(accum_ptr: int, prev_ptr: int, pixel_count: int, in_ptr: int | None, n_in: int,
                        sel: RtcSelectDesc, out_ptr: int | None, capacity: int, count_ptr: int | None,
                        samples_ptr: int | None, scratch_ptr: int, scratch_bytes: int, stream: int | None = None) -> None:
    """rtc_select_pixels_async on the current device (include/rtc.h): addresses as ints, 0 or None for a null pointer."""
    check(lib().rtc_select_pixels_async(_vp(accum_ptr), _vp(prev_ptr), int(pixel_count), _vp(in_ptr), int(n_in),
                                        C.byref(sel), _vp(out_ptr), int(capacity), _vp(count_ptr), _vp(samples_ptr),
                                        _vp(scratch_ptr), int(scratch_bytes), _vp(stream)), "rtc_select_pixels_async")


def resolve_async(accum_ptr: int, samples_ptr: int, pixel_count: int, spp: int, colors_ptr: int,
                  stream: int | None = None) -> None:
    """rtc_resolve_async on the current device (include/rtc.h): colors at any byte alignment."""
    check(lib().rtc_resolve_async(_vp(accum_ptr), _vp(samples_ptr), int(pixel_count), int(spp), _vp(colors_ptr),
                                  _vp(stream)), "rtc_resolve_async")


def _frame_tensor(who: str, name: str, t, dev, nbytes: int, dtype=None):
    if not hasattr(t, "data_ptr") or not t.is_cuda or t.device != dev or not t.is_contiguous() or \
            t.numel() * t.element_size() != nbytes or (dtype is not None and t.dtype != dtype):
        raise ValueError(f"{who}: {name} must be a contiguous tensor of {nbytes} bytes on the accumulator's device")
    return t


def _accum_pixels(who: str, accum, what: str = "accum is float32, three per pixel") -> int:
    """A device accumulator's pixel count: a contiguous float32 tensor of three floats per pixel (`what`: the refusal of
    another type or size)."""
    import torch

    if accum.dtype != torch.float32 or accum.numel() % 3:
        raise ValueError(f"{who}: {what}")
    npix = accum.numel() // 3
    _frame_tensor(who, "accum", accum, accum.device, 12 * npix)
    return npix


def _scratch(nbytes: int, dev):
    """A torch allocation of at least nbytes (and at least 16: an empty tensor has no address) bytes on `dev`."""
    import torch

    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def select_pixels(accum, prev, sel: RtcSelectDesc, pixels=None, capacity: int | None = None, samples=None):
    """The pixels of a progressive frame that go on (include/rtc.h): (out, count).  `accum` and `prev` are the
    accumulator now and its snapshot at an earlier sample count, float32 of 3 floats per pixel; `pixels` the input list
    (compact indices; None: every pixel; an entry >= the pixel count is skipped); `out` holds the selected entries in
    input order, cut at `capacity` (None: the input's length) and filled up with 0xFFFFFFFF, `count` the number selected
    before the cut; `samples` (int32, one per pixel), where given, gets sel.samplesDone IN PLACE at every valid entry.
    Everything numpy: rtc_select_pixels_host, anywhere; out uint32 [capacity], count an int.  Everything a contiguous torch
    tensor on one device: rtc_select_pixels_async on torch's current stream there with a torch allocation as scratch, no
    synchronisation; out int32 [capacity] (the same bits) and count int64 [1] are device tensors."""
    who = "select_pixels"
    if hasattr(accum, "data_ptr"):
        import torch

        dev = accum.device
        npix = _accum_pixels(who, accum)
        _frame_tensor(who, "prev", prev, dev, 12 * npix, torch.float32)
        if samples is not None:
            _frame_tensor(who, "samples", samples, dev, 4 * npix, torch.int32)
        n_in = 0
        if pixels is not None:
            n_in = pixels.numel() if hasattr(pixels, "data_ptr") else -1
            _frame_tensor(who, "pixels", pixels, dev, 4 * max(n_in, 0))
        n = npix if pixels is None else n_in
        capacity = n if capacity is None else int(capacity)
        out = torch.empty(capacity, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        nbytes = select_scratch_bytes(n)
        scratch = _scratch(nbytes, dev)
        with _stream_of(dev) as st:
            select_pixels_async(accum.data_ptr(), prev.data_ptr(), npix, None if pixels is None else pixels.data_ptr(),
                                n_in, sel, out.data_ptr() if capacity else None, capacity, count.data_ptr(),
                                None if samples is None else samples.data_ptr(), scratch.data_ptr(), nbytes,
                                st.cuda_stream)
        return out, count
    acc = np.ascontiguousarray(accum, np.float32).reshape(-1)
    prv = np.ascontiguousarray(prev, np.float32).reshape(-1)
    if acc.size % 3 or prv.size != acc.size:
        raise ValueError(f"{who}: accum and prev are float32, three per pixel, of one frame")
    npix = acc.size // 3
    if samples is not None and (not isinstance(samples, np.ndarray) or samples.dtype != np.int32 or samples.size != npix
                                or not samples.flags.c_contiguous):
        raise ValueError(f"{who}: samples must be a contiguous int32 array of the frame's {npix} pixels")
    px = None
    if pixels is not None:
        px = np.asarray(pixels).reshape(-1)
        if px.size and (not np.issubdtype(px.dtype, np.integer) or px.min() < 0 or px.max() > 0xffffffff):
            raise ValueError(f"{who}: pixels must be integers in [0, 2^32)")
        px = np.ascontiguousarray(px, np.uint32)
    n = npix if px is None else len(px)
    capacity = n if capacity is None else int(capacity)
    out = np.zeros(capacity, np.uint32)
    count = C.c_ulonglong(0)
    stand_in = np.zeros(1, np.float32)  # (an empty numpy array has no address to speak of)
    check(lib().rtc_select_pixels_host(_ptr(acc if npix else stand_in), _ptr(prv if npix else stand_in), npix,
                                       None if px is None else _ptr(px if len(px) else np.zeros(1, np.uint32)), n if px is not None else 0,
                                       C.byref(sel), _ptr(out) if capacity else None, capacity,
                                       C.cast(C.pointer(count), C.c_void_p), _ptr(samples)), "rtc_select_pixels_host")
    return out, int(count.value)


def resolve(accum, samples, spp: int):
    """The displayable frame of an adaptive render (include/rtc.h): uint8 of accum's shape, floatToUint(accum * spp /
    samples) per component (0 where samples <= 0).  numpy arrays: rtc_resolve_host, anywhere; contiguous torch tensors on
    one device: rtc_resolve_async on torch's current stream there, no synchronisation."""
    who = "resolve"
    if hasattr(accum, "data_ptr"):
        import torch

        dev = accum.device
        npix = _accum_pixels(who, accum)
        _frame_tensor(who, "samples", samples, dev, 4 * npix, torch.int32)
        colors = torch.empty(accum.shape, dtype=torch.uint8, device=dev)
        if npix:
            with _stream_of(dev) as st:
                resolve_async(accum.data_ptr(), samples.data_ptr(), npix, spp, colors.data_ptr(), st.cuda_stream)
        return colors
    acc = np.ascontiguousarray(accum, np.float32)
    smp = np.ascontiguousarray(samples, np.int32)
    if acc.size % 3 or smp.size * 3 != acc.size:
        raise ValueError(f"{who}: accum float32, three per pixel, and samples int32, one per pixel")
    colors = np.zeros(acc.shape, np.uint8)
    if acc.size:
        check(lib().rtc_resolve_host(_ptr(acc), _ptr(smp), smp.size, int(spp), _ptr(colors)), "rtc_resolve_host")
    elif int(spp) <= 0:
        raise ValueError(f"{who}: spp = {spp}")
    return colors


def denoise_desc(width: int, rows: int, iterations: int = 5, normal_squarings: int = 5, depth_scale: float = 1.0,
                 color_scale: float = 1.0, albedo_floor: float = 0.0, demodulate: bool = False,
                 spp: int = 0) -> RtcDenoiseDesc:
    """The RtcDenoiseDesc of a rows x width frame (include/rtc.h): `iterations` a-trous iterations (steps 1,
    2, 4, ...), the normal weight max(0, n.nq) ^ (2 ^ normal_squarings), the depth weight 1 / (1 + ((z - zq) *
    depth_scale)^2), the colour weight 1 / (1 + e^2 * color_scale * 4^k) with e the L1 colour distance; demodulate:
    RTC_DN_DEMODULATE (the colour is divided by the albedo where that exceeds albedo_floor, filtered, and multiplied
    again).  The three floats are rounded to f32 once; spp counts only with per-pixel sample counts."""
    return RtcDenoiseDesc(int(width), int(rows), int(iterations), RTC_DN_DEMODULATE if demodulate else 0, int(spp),
                          int(normal_squarings), float(depth_scale), float(color_scale), float(albedo_floor))


def denoise_scratch_bytes(n: int, iterations: int) -> int:
    """rtc_denoise_scratch_bytes: the device scratch rtc_denoise_async needs for n pixels and `iterations` iterations."""
    return int(lib().rtc_denoise_scratch_bytes(int(n), int(iterations)))


def denoise_async(accum_ptr: int, samples_ptr: int | None, desc: RtcDenoiseDesc, out_ptr: int, colors_ptr: int | None,
                  scratch_ptr: int, scratch_bytes: int, normal_ptr: int | None = None, depth_ptr: int | None = None,
                  albedo_ptr: int | None = None, stream: int | None = None) -> None:
    """rtc_denoise_async on the current device (include/rtc.h): addresses as ints, 0 or None for a null pointer."""
    guides = RtcHitBuffers(None, depth_ptr or None, normal_ptr or None, albedo_ptr or None)
    check(lib().rtc_denoise_async(_vp(accum_ptr), _vp(samples_ptr), C.byref(guides), C.byref(desc), _vp(out_ptr),
                                  _vp(colors_ptr), _vp(scratch_ptr), int(scratch_bytes), _vp(stream)), "rtc_denoise_async")


_GUIDE_FLOATS = {"normal": 3, "depth": 1, "albedo": 3}


def denoise(accum, guides=None, samples=None, spp=None, desc: RtcDenoiseDesc | None = None, colors: bool = False):
    """A frame's accumulator through the edge-avoiding a-trous filter (include/rtc.h): float32 of accum's
    shape, or (that, uint8 of accum's shape: floatToUint of it) with colors=True.  `accum`: float32 [rows, W, 3]; `guides`:
    the dict DeviceScene.first_hit returns or its device tensors -- "normal", "depth" and "albedo" are used where present
    (albedo only with a demodulating desc), "prim" is ignored; `samples` (int32 [rows, W]) and `spp`: the per-pixel sample
    counts and the frame's spp of an adaptive render (DeviceScene.render_adaptive_device), so that every pixel is scaled by
    spp / samples first; `desc`: denoise_desc(...) for accum's width and rows (None: denoise_desc(W, rows)).
    Everything numpy: rtc_denoise_host, anywhere, no GPU.  Everything a contiguous torch tensor on one device:
    rtc_denoise_async on torch's current stream there with a torch allocation as scratch, no synchronisation."""
    who = "denoise"
    on_device = hasattr(accum, "data_ptr")
    shape = tuple(accum.shape)
    if len(shape) != 3 or shape[2] != 3 or shape[0] <= 0 or shape[1] <= 0:
        raise ValueError(f"{who}: accum is float32 [rows, W, 3], not {shape}")
    rows, width = shape[0], shape[1]
    npix = rows * width
    if desc is None:
        desc = denoise_desc(width, rows)
    if (desc.width, desc.rows) != (width, rows):
        raise ValueError(f"{who}: the desc is for {desc.width} x {desc.rows}, accum for {width} x {rows}")
    if (samples is None) != (spp is None):
        raise ValueError(f"{who}: samples and spp go together")
    d = RtcDenoiseDesc.from_buffer_copy(desc)
    if spp is not None:
        d.spp = int(spp)
    guides = {k: v for k, v in (guides or {}).items() if k in _GUIDE_FLOATS and v is not None}
    if not d.flags & RTC_DN_DEMODULATE:
        guides.pop("albedo", None)
    if on_device:
        import torch

        dev = accum.device
        _accum_pixels(who, accum, "accum is float32")
        if samples is not None:
            _frame_tensor(who, "samples", samples, dev, 4 * npix, torch.int32)
        for k, v in guides.items():
            _frame_tensor(who, k, v, dev, 4 * _GUIDE_FLOATS[k] * npix, torch.float32)
        out = torch.empty_like(accum)
        col = torch.empty(shape, dtype=torch.uint8, device=dev) if colors else None
        nbytes = denoise_scratch_bytes(npix, d.iterations)
        scratch = _scratch(nbytes, dev)
        with _stream_of(dev) as st:
            denoise_async(accum.data_ptr(), None if samples is None else samples.data_ptr(), d, out.data_ptr(),
                          None if col is None else col.data_ptr(), scratch.data_ptr(), nbytes,
                          **{k + "_ptr": v.data_ptr() for k, v in guides.items()}, stream=st.cuda_stream)
        return (out, col) if colors else out
    acc = np.ascontiguousarray(accum, np.float32)
    smp = None
    if samples is not None:
        smp = np.ascontiguousarray(samples, np.int32)
        if smp.size != npix:
            raise ValueError(f"{who}: samples is int32, one per pixel")
    held = {}
    for k, v in guides.items():
        held[k] = np.ascontiguousarray(v, np.float32)
        if held[k].size != _GUIDE_FLOATS[k] * npix:
            raise ValueError(f"{who}: guides[{k!r}] has {held[k].size} floats for {npix} pixels")
    hb = RtcHitBuffers(None, _ptr(held.get("depth")), _ptr(held.get("normal")), _ptr(held.get("albedo")))
    out = np.zeros(shape, np.float32)
    col = np.zeros(shape, np.uint8) if colors else None
    check(lib().rtc_denoise_host(_ptr(acc), _ptr(smp), C.byref(hb), C.byref(d), _ptr(out), _ptr(col)), "rtc_denoise_host")
    return (out, col) if colors else out


def save_progress(path: str, state: ProgressState) -> None:
    """Write a progressive frame's state as an .npz on the host (np.savez: `path` gets the suffix when it lacks it), so
    that a later process can finish the frame (load_progress, render_progressive(..., state=...)) bit-identically."""
    np.savez(path, accum=np.ascontiguousarray(state.accum, np.float32), rng=np.ascontiguousarray(state.rng, np.uint32),
             samples_done=np.int64(state.samples_done), cfg_keys=np.array(list(state.cfg)),
             cfg_values=np.array([state.cfg[k] for k in state.cfg], np.int64))


def load_progress(path: str) -> ProgressState:
    """The ProgressState save_progress wrote."""
    with np.load(path) as z:
        cfg = {str(k): int(v) for k, v in zip(z["cfg_keys"], z["cfg_values"])}
        return ProgressState(z["accum"].astype(np.float32), z["rng"].astype(np.uint32), int(z["samples_done"]), cfg)


def copy_async(dst_ptr: int, src_ptr: int, nbytes: int, blocks: int = 32, stream: int | None = None) -> None:
    """rtc_copy_async: a copy with a small CU footprint (e.g. Color[] into pinned host memory)."""
    check(lib().rtc_copy_async(C.c_void_p(dst_ptr), C.c_void_p(src_ptr), C.c_size_t(nbytes), int(blocks),
                               C.c_void_p(stream) if stream else None), "rtc_copy_async")


def ray_keys_host(rays, lo, hi) -> np.ndarray:
    """rtc_ray_keys_host (no GPU): the 30-bit coherence keys of `rays` (RAY_DT [n] or float32 [n, 6]) in the box lo, hi
    (three floats each) as uint32 [n] -- the host statement of the key the device sort uses."""
    _, a, n = _query_rays("ray_keys_host", np.asarray(rays))
    lo, hi = (np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1)) for v in (lo, hi))
    if lo.size != 3 or hi.size != 3:
        raise ValueError("ray_keys_host: lo and hi are three floats each")
    keys = np.zeros(n, np.uint32)
    check(lib().rtc_ray_keys_host(_ptr(a) if n else None, n, _ptr(lo), _ptr(hi), _ptr(keys) if n else None),
          "rtc_ray_keys_host")
    return keys


def ray_order_scratch_bytes(n: int) -> int:
    """rtc_ray_order_scratch_bytes: the device scratch rtc_ray_order_async needs for n rays."""
    return int(lib().rtc_ray_order_scratch_bytes(int(n)))


def gather_async(dst_ptr: int, src_ptr: int, order_ptr: int, n: int, elem_bytes: int, stream: int | None = None) -> None:
    """rtc_gather_async: dst[i] = src[order[i]] for n elements of elem_bytes (1, or a multiple of 4 up to 64) on the
    current device; dst must not alias src."""
    check(lib().rtc_gather_async(_vp(dst_ptr), _vp(src_ptr), _vp(order_ptr), n, elem_bytes, _vp(stream)),
          "rtc_gather_async")


def scatter_async(dst_ptr: int, src_ptr: int, order_ptr: int, n: int, elem_bytes: int, stream: int | None = None) -> None:
    """rtc_scatter_async: dst[order[i]] = src[i], the inverse of gather_async with the same order."""
    check(lib().rtc_scatter_async(_vp(dst_ptr), _vp(src_ptr), _vp(order_ptr), n, elem_bytes, _vp(stream)),
          "rtc_scatter_async")


def copy_d2h_dma(host_ptr: int, dev_ptr: int, nbytes: int) -> None:
    """rtc_copy_d2h_dma: device -> page-locked host memory on the SDMA engines, blocking (GIL released)."""
    check(lib().rtc_copy_d2h_dma(C.c_void_p(host_ptr), C.c_void_p(dev_ptr), C.c_size_t(nbytes)), "rtc_copy_d2h_dma")


def copy_rows_d2h_dma(host_ptr: int, host_pitch: int, dev_ptr: int, src_pitch: int, row_bytes: int, rows: int) -> None:
    """rtc_copy_rows_d2h_dma: rows of device memory into page-locked host memory with a row pitch (SDMA, blocking):
    a rank's interleaved rows straight into their places of the host frame."""
    check(lib().rtc_copy_rows_d2h_dma(C.c_void_p(host_ptr), C.c_size_t(host_pitch), C.c_void_p(dev_ptr),
                                      C.c_size_t(src_pitch), C.c_size_t(row_bytes), int(rows)), "rtc_copy_rows_d2h_dma")


def host_register(ptr: int, nbytes: int) -> None:
    """rtc_host_register: page-lock an existing host range (e.g. a shared-memory frame every rank maps)."""
    check(lib().rtc_host_register(C.c_void_p(ptr), C.c_size_t(nbytes)), "rtc_host_register")


def host_unregister(ptr: int) -> None:
    """rtc_host_unregister; raises RtcError(RTC_EBUSY) while a timed-out copy may still write the range."""
    check(lib().rtc_host_unregister(C.c_void_p(ptr)), "rtc_host_unregister")


def dma_pending(ptr: int | None = None, nbytes: int = 0) -> int:
    """rtc_dma_pending: copies that timed out (RTC_ETIMEDOUT) and may still read or write [ptr, ptr + nbytes)
    (None: any range).  Buffers they touch must not be freed or reused while this is > 0."""
    n = lib().rtc_dma_pending(C.c_void_p(ptr) if ptr else None, C.c_size_t(nbytes if ptr else 0))
    if n < 0:
        check(n, "rtc_dma_pending")
    return n


def deinterleave_async(compact_ptr: int, parts: int, rows_per_part: int, width: int, height: int, out_ptr: int,
                       stream: int | None = None, row_band: int = 1):
    """rtc_deinterleave_async (single rows) / rtc_deinterleave_bands_async (bands of row_band rows)."""
    if row_band > 1:
        check(lib().rtc_deinterleave_bands_async(C.c_void_p(compact_ptr), parts, rows_per_part, width, height, row_band,
                                                 C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None),
              "rtc_deinterleave_bands_async")
        return
    check(lib().rtc_deinterleave_async(C.c_void_p(compact_ptr), parts, rows_per_part, width, height,
                                       C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None),
          "rtc_deinterleave_async")


def bounce_hit_share(tris, spheres=None) -> float:
    """rtc_bounce_hit_share: the share of diffuse bounce rays from the triangles that hit the scene again (host probe,
    a scheduling hint).  With `spheres` (rtc_bounce_hit_share_all): the rays start on the triangles and the spheres,
    area-weighted, and are tested against both -- the value the sphere split's gate compares."""
    t, nt = _arr(tris, TRIANGLE_DT)
    out = C.c_float()
    if spheres is None:
        check(lib().rtc_bounce_hit_share(_ptr(t), nt, C.byref(out)), "rtc_bounce_hit_share")
        return out.value
    s, ns = _arr(spheres, SPHERE_DT)
    check(lib().rtc_bounce_hit_share_all(_ptr(t), nt, _ptr(s), ns, C.byref(out)), "rtc_bounce_hit_share_all")
    return out.value


def vec3ToColor(accum: np.ndarray) -> np.ndarray:
    """raytracing.c:11-15 / moremath.c:25-30 on a float3 buffer (host)."""
    a = np.ascontiguousarray(accum, dtype=np.float32)
    out = np.empty(a.shape, np.uint8)
    check(lib().rtc_quantize(_ptr(a), a.size // 3, _ptr(out)), "rtc_quantize")
    return out


def write_bmp(path: str, colors: np.ndarray) -> None:
    """stbi_write_bmp(path, W, H, 3, image) (main.c:305)."""
    c = np.ascontiguousarray(colors, dtype=np.uint8)
    h, w = c.shape[0], c.shape[1]
    check(lib().rtc_write_bmp(path.encode(), w, h, _ptr(c)), "rtc_write_bmp")


def device_count() -> int:
    n = C.c_int()
    rc = lib().rtc_device_count(C.byref(n))
    return n.value if rc == 0 else 0


# ---- device probes (same device code as the renderer) --------------------------------------------------
def rayTriangle(rays: np.ndarray, tris: np.ndarray):
    """raytracing.c:186-214 on the GPU, one (ray, triangle) pair per element -> (didHit int32, dst f32)."""
    r = np.ascontiguousarray(rays, RAY_DT)
    t = np.ascontiguousarray(tris, TRIANGLE_DT)
    n = len(r)
    hit, dst = np.zeros(n, np.int32), np.zeros(n, np.float32)
    check(lib().rtc_probe_ray_triangle(_ptr(r), _ptr(t), n, _ptr(hit), _ptr(dst)), "rtc_probe_ray_triangle")
    return hit, dst


def raySphere(rays: np.ndarray, spheres: np.ndarray):
    """raytracing.c:162-184 on the GPU -> (didHit, dst, normal[n,3])."""
    r = np.ascontiguousarray(rays, RAY_DT)
    s = np.ascontiguousarray(spheres, SPHERE_DT)
    n = len(r)
    hit, dst, nrm = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    check(lib().rtc_probe_ray_sphere(_ptr(r), _ptr(s), n, _ptr(hit), _ptr(dst), _ptr(nrm)), "rtc_probe_ray_sphere")
    return hit, dst, nrm


def getEnvironmentLight(rays: np.ndarray, scenes: np.ndarray) -> np.ndarray:
    """raytracing.c:151-160 on the GPU -> float32 [n, 3]."""
    r = np.ascontiguousarray(rays, RAY_DT)
    s = np.ascontiguousarray(scenes, SCENE_DT)
    n = len(r)
    out = np.zeros((n, 3), np.float32)
    check(lib().rtc_probe_environment(_ptr(r), _ptr(s), n, _ptr(out)), "rtc_probe_environment")
    return out


def sky_miss_probe(rays: np.ndarray, scene, spp: int = 1):
    """The sky kernel's per-pixel sun skip on the GPU for one scene, with the limit and gating a launch computes on the
    host: (vanish int32 [n], environment float32 [n, 3] evaluated with it, the sky kernel's pixel sum float32 [n, 3] of spp
    camera-ray misses)."""
    r = np.ascontiguousarray(rays, RAY_DT)
    s = np.ascontiguousarray(scene, SCENE_DT).reshape(1)
    n = len(r)
    v = np.zeros(n, np.int32)
    out = np.zeros((n, 3), np.float32)
    acc = np.zeros((n, 3), np.float32)
    check(lib().rtc_probe_sun_vanish(_ptr(r), _ptr(s), n, spp, _ptr(v), _ptr(out), _ptr(acc)), "rtc_probe_sun_vanish")
    return v, out, acc


def sun_vanish_probe(rays: np.ndarray, scenes: np.ndarray):
    """sky_miss_probe's (vanish, environment) for one scene, given once or once per ray (the probe runs one scene per
    launch, as a render does)."""
    s = np.ascontiguousarray(scenes, SCENE_DT).reshape(-1)
    if len(s) == 0 or s.tobytes() != s[:1].tobytes() * len(s):  # (bytes: a NaN intensity equals itself)
        raise ValueError("sun_vanish_probe: one scene per call")
    return sky_miss_probe(rays, s[0], 1)[:2]


def env_vanish_limit(scene) -> float:
    """The bound on focus * log2(x) below which the sky kernel skips the sun term (host only; -inf: never)."""
    s = np.ascontiguousarray(scene, SCENE_DT).reshape(1)
    out = C.c_double(0.0)
    check(lib().rtc_env_vanish_limit(_ptr(s), C.byref(out)), "rtc_env_vanish_limit")
    return out.value


def random_sequences(seeds: np.ndarray, draws: int):
    """moremath.c:89-108 on the GPU: per seed, `draws` x RandomValue, x RandomValueNormalDistrubtion and
    x RandomDiretion, each sequence restarted from the seed."""
    sd = np.ascontiguousarray(seeds, np.uint32)
    n = len(sd)
    u = np.zeros((n, draws), np.float32)
    g = np.zeros((n, draws), np.float32)
    d = np.zeros((n, draws, 3), np.float32)
    check(lib().rtc_probe_random(_ptr(sd), n, draws, _ptr(u), _ptr(g), _ptr(d)), "rtc_probe_random")
    return u, g, d


def cluster_bound_probe(tris: np.ndarray, rays: np.ndarray) -> dict:
    """Soundness of the bounce-ray cluster culling on the GPU (rtc_probe_cluster_bound): hits inside culled
    clusters (must be 0), clusters culled, cluster tests, hits, largest hit excess over a bounding radius; hits
    on triangles the first-bounce reach mask calls unreachable from the ray's origin (must be 0), pairs so called."""
    t = np.ascontiguousarray(tris, TRIANGLE_DT)
    r = np.ascontiguousarray(rays, RAY_DT)
    c = np.zeros(7, np.uint64)
    check(lib().rtc_probe_cluster_bound(_ptr(t), len(t), _ptr(r), len(r), _ptr(c)), "rtc_probe_cluster_bound")
    return {"violations": int(c[0]), "culled": int(c[1]), "tests": int(c[2]), "hits": int(c[3]),
            "max_excess": float(np.array([c[4]], np.uint64).astype(np.uint32).view(np.float32)[0]),
            "reach_violations": int(c[5]), "unreachable": int(c[6])}


def item_records_probe(tris, spheres, scene: Scene, cam: RtcCamera, cfg: RenderConfig) -> dict:
    """The split launch's item records for the launch `cfg` (rtc_probe_item_records: its preparation and culls, no render
    kernel): counts [16] the sub-lists' entries, records uint32 [n, 4] (dword 0 = x | launch row << 16, or tile * 64 + bit
    when `wide`; dwords 1-3 the float bits of the pixel's primary direction), pix_mask uint64 [tiles], and the launch's
    cap (entries a sub-list holds), tiles_x, tiles, wide."""
    t, nt = _arr(tris, TRIANGLE_DT)
    s, ns = _arr(spheres, SPHERE_DT)
    rows = cfg.rows()
    tiles = 4 * ((cfg.width + 15) // 16) * ((rows + 15) // 16)
    counts, info = np.zeros(16, np.int32), np.zeros(4, np.int32)
    rec = np.zeros((tiles * 64, 4), np.uint32)
    pm = np.zeros(tiles, np.uint64)
    d = cfg.desc()
    check(lib().rtc_probe_item_records(_ptr(t), nt, _ptr(s), ns, C.byref(scene), C.byref(cam), C.byref(d), _ptr(counts),
                                       _ptr(info), _ptr(rec), len(rec), _ptr(pm), len(pm)), "rtc_probe_item_records")
    return {"counts": counts, "records": rec[: int(counts.sum())].copy(), "pix_mask": pm, "cap": int(info[0]),
            "tiles_x": int(info[1]), "tiles": int(info[2]), "wide": bool(info[3])}


def primary_cull_probe(tris, scene: Scene, cam: RtcCamera, cfg: RenderConfig) -> dict:
    """The primary cull of the launch `cfg` (rtc_probe_primary_cull: its preparation and culls, no render kernel): kept
    uint8 [rows, width, triangles] the per-pixel filter's verdict for every triangle, tile_bits uint64 [tiles, words] the
    tiles' candidate bit-sets, pix_mask uint64 [tiles], and tiles, tiles_x, words, level0 (the superblock level ran); prim_f
    float32 [triangles, 16] the launch's filter records (DevPrimF), cones float64 [tiles, 4] the tiles' prefilter {eDir,
    vmin, vmax, usable} and pruned uint8 [tiles, triangles] the tiles' own prefilter verdicts."""
    t, nt = _arr(tris, TRIANGLE_DT)
    rows = cfg.rows()
    tiles = 4 * ((cfg.width + 15) // 16) * ((rows + 15) // 16)
    words = ((nt + 7) // 8 * 8 + 63) // 64
    kept = np.zeros((rows, cfg.width, nt), np.uint8)
    bits = np.zeros((tiles, words), np.uint64)
    pm = np.zeros(tiles, np.uint64)
    info = np.zeros(4, np.int32)
    prim_f = np.zeros((nt, 16), np.float32)
    cones = np.zeros((tiles, 4), np.float64)
    pruned = np.zeros((tiles, nt), np.uint8)
    d = cfg.desc()
    check(lib().rtc_probe_primary_cull(_ptr(t), nt, C.byref(scene), C.byref(cam), C.byref(d), _ptr(kept), kept.size,
                                       _ptr(bits), bits.size, _ptr(pm), len(pm), _ptr(info), _ptr(prim_f), _ptr(cones),
                                       _ptr(pruned)), "rtc_probe_primary_cull")
    assert int(info[0]) == tiles and int(info[2]) == words, info
    return {"kept": kept, "tile_bits": bits, "pix_mask": pm, "tiles": int(info[0]), "tiles_x": int(info[1]),
            "words": int(info[2]), "level0": bool(info[3]), "prim_f": prim_f, "cones": cones, "pruned": pruned}
