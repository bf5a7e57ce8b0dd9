"""The edge-avoiding a-trous filter of rtc_denoise_async / rtc_denoise_host (include/rtc.h) restated in numpy,
with no code under test in the loop, the shapes and the designed inputs both are held to, and the frames the property
tests use.

The statement, float32 operation by operation (numpy rounds every float32 operation to float32 and keeps subnormals), one
vectorised numpy operation per operation of the statement:
    load:       L = A, or A * (s > 0 ? spp / s : 0) with sample counts; with DEMODULATE L_c = a_c > floor ? L_c / a_c : L_c
    iteration:  sum = c * 0.140625, wsum = 0.140625; the other 24 taps j = -2 .. 2 outer, i = -2 .. 2 inner, step 1 << k,
                a tap outside the image skipped: w = H[|i|] * H[|j|]; the normal weight max(0, n.nq) squared
                normalSquarings times; the depth weight 1 / (1 + ((z - zq) * depthScale)^2); the colour weight
                1 / (1 + e * e * colorScale * 4^k), e the L1 distance; !(w > 0) skipped; sum += q * w, wsum += w;
                C' = sum / wsum
    store:      O_c = a_c > floor ? C'_c * a_c : C'_c with DEMODULATE; the Color byte floatToUint(O_c)"""
from __future__ import annotations

import types

import numpy as np

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
H = (F(0.375), F(0.25), F(0.0625))
W0 = F(0.140625)
DEMODULATE = 0x1
MISS_DEPTH = F(999999.0)

FIXED_SHAPES = ((1, 1), (1, 70), (70, 1), (5, 3), (31, 33), (64, 64), (65, 63), (129, 67))  # (W, rows)
GUIDE_SUBSETS = ("none", "normal", "depth", "both", "albedo")  # albedo: both guides, an albedo buffer and DEMODULATE


DIRECT_ROWS = 8  # from step 4 on a workgroup takes tileW x 8 pixels (include/rtc.h)


def shapes(tile_w, tile_h):
    """(W, rows): the fixed set; W and rows at tile - 1, tile, tile + 1 and 2 tile + 1 (a few rows or columns beside them:
    the other axis is covered by the fixed set and by the square case); rows around the 8 of the kernel without LDS; and a
    long row and a long column of 8 tiles and one pixel (first built for a tiling by residue class, where the sub-lattices
    of step 4 are then of unequal length; kept as the widest cases)."""
    out = list(FIXED_SHAPES)
    for w in (tile_w - 1, tile_w, tile_w + 1, 2 * tile_w + 1):
        out.append((w, 7))
    for r in (tile_h - 1, tile_h, tile_h + 1, 2 * tile_h + 1, DIRECT_ROWS, DIRECT_ROWS + 1, 2 * DIRECT_ROWS + 1):
        out.append((6, r))
    out.append((tile_w + 1, tile_h + 1))
    out.append((2 * 4 * tile_w + 1, 5))
    out.append((5, 2 * 4 * tile_h + 1))
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return tuple(uniq)


def desc(width, rows, iterations, flags=0, spp=0, normal_squarings=0, depth_scale=1.0, color_scale=1.0, albedo_floor=0.0):
    """The nine fields of an RtcDenoiseDesc, the three floats rounded to float32 once."""
    return types.SimpleNamespace(width=int(width), rows=int(rows), iterations=int(iterations), flags=int(flags),
                                 spp=int(spp), normalSquarings=int(normal_squarings), depthScale=F(depth_scale),
                                 colorScale=F(color_scale), albedoFloor=F(albedo_floor))


def load(accum, d, samples=None, albedo=None):
    L = np.array(accum, F).reshape(d.rows, d.width, 3)
    with np.errstate(all="ignore"):
        if samples is not None:
            s = np.asarray(samples, np.int32).reshape(d.rows, d.width)
            scale = np.where(s > 0, F(d.spp) / s.astype(F), F(0))
            assert scale.dtype == F
            L = L * scale[:, :, None]
        if d.flags & DEMODULATE:
            a = np.asarray(albedo, F).reshape(d.rows, d.width, 3)
            L = np.where(a > d.albedoFloor, L / a, L)
    assert L.dtype == F
    return L


def iteration(C, d, k, normal=None, depth=None):
    """One iteration with step 1 << k over C float32 [rows, W, 3]."""
    rows, width = d.rows, d.width
    s = 1 << k
    cs = d.colorScale * F(1 << (2 * k))
    with np.errstate(all="ignore"):
        total = C * W0
        wsum = np.full((rows, width), W0, F)
        for j in range(-2, 3):
            for i in range(-2, 3):
                if i == 0 and j == 0:
                    continue
                y0, y1 = max(0, -j * s), min(rows, rows - j * s)  # the centres whose tap lies inside the image
                x0, x1 = max(0, -i * s), min(width, width - i * s)
                if y0 >= y1 or x0 >= x1:
                    continue
                here = (slice(y0, y1), slice(x0, x1))
                there = (slice(y0 + j * s, y1 + j * s), slice(x0 + i * s, x1 + i * s))
                c, q = C[here], C[there]
                w = np.full(c.shape[:2], H[abs(i)] * H[abs(j)], F)
                if normal is not None:
                    n, nq = normal[here], normal[there]
                    t = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    t = np.where(t > 0, t, F(0))
                    for _ in range(d.normalSquarings):
                        t = t * t
                    w = w * t
                if depth is not None:
                    dz = (depth[here] - depth[there]) * d.depthScale
                    w = w / (F(1) + dz * dz)
                e = (np.abs(c[..., 0] - q[..., 0]) + np.abs(c[..., 1] - q[..., 1])) + np.abs(c[..., 2] - q[..., 2])
                w = w / (F(1) + (e * e) * cs)
                assert w.dtype == e.dtype == F
                enters = w > 0
                total[here] = np.where(enters[..., None], total[here] + q * w[..., None], total[here])
                wsum[here] = np.where(enters, wsum[here] + w, wsum[here])
        out = total / wsum[:, :, None]
    assert out.dtype == F
    return out


def denoise(accum, d, samples=None, normal=None, depth=None, albedo=None):
    """float32 [rows, W, 3]: what rtc_denoise_host writes to `out`."""
    normal = None if normal is None else np.asarray(normal, F).reshape(d.rows, d.width, 3)
    depth = None if depth is None else np.asarray(depth, F).reshape(d.rows, d.width)
    C = load(accum, d, samples, albedo)
    for k in range(d.iterations):
        C = iteration(C, d, k, normal, depth)
    if d.flags & DEMODULATE:
        a = np.asarray(albedo, F).reshape(d.rows, d.width, 3)
        with np.errstate(all="ignore"):
            C = np.where(a > d.albedoFloor, C * a, C)
    assert C.dtype == F
    return C


def quantize(v):
    """floatToUint (moremath.c:25-30) per component: below 0 -> 0, 1 and above -> 255, NaN -> 0, else (unsigned)(f * 255)"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        scaled = np.where((v >= 0) & (v < 1), v * F(255), F(0))
        out = scaled.astype(np.uint8)
    out[v >= 1] = 255
    return out


# ---- frames ---------------------------------------------------------------------------------------------------------
def _ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, INF if k > 0 else -INF, dtype=F)
    return x


def random_frame(seed, width, rows, spp=12):
    """A seeded frame with every buffer: colours around a few levels, three kinds of surfaces (unit normals), a band of
    first-hit misses (normal +0, depth 999999), albedos around the floors the tests use, and sample counts."""
    r = np.random.RandomState(seed)
    n = width * rows
    acc = (r.rand(rows, width, 3) * r.choice([0.05, 0.5, 1.0, 3.0], (rows, width, 1))).astype(F)
    faces = np.array([(0, 0, 1), (0, 1, 0), (0.6, 0, 0.8), (0, 0, 0)], F)
    which = (r.randint(0, 3, (rows, width)) if n < 64 else
             ((np.arange(width)[None, :] * 3 // max(width, 1)) + (np.arange(rows)[:, None] * 2 // max(rows, 1))) % 3)
    miss = r.rand(rows, width) < 0.08
    which = np.where(miss, 3, which)
    normal = faces[which]
    depth = np.where(miss, MISS_DEPTH, (2 + 4 * r.rand(rows, width) + which)).astype(F)
    albedo = r.choice(np.array([0, 0.01, 0.25, 0.5, 0.73, 1.0], F), (rows, width, 3)).astype(F)
    albedo[miss] = 0
    samples = r.choice(np.array([0, 1, spp // 2, spp], np.int32), (rows, width), p=[0.02, 0.08, 0.4, 0.5]).astype(np.int32)
    return dict(accum=acc, samples=samples, spp=spp, normal=normal, depth=depth, albedo=albedo)


def guide_args(frame, subset):
    """(keyword arguments of `denoise` beyond accum and desc, desc flags) for a guide subset of a frame"""
    kw = {}
    if subset in ("normal", "both", "albedo"):
        kw["normal"] = frame["normal"]
    if subset in ("depth", "both", "albedo"):
        kw["depth"] = frame["depth"]
    if subset == "albedo":
        kw["albedo"] = frame["albedo"]
    return kw, (DEMODULATE if subset == "albedo" else 0)


def designed_frames():
    """name -> (frame, desc keyword arguments): small frames with the values the statement's branches turn on."""
    out = {}
    W, R = 11, 9

    def base(seed):
        f = random_frame(seed, W, R)
        f["normal"] = np.tile(np.array((0, 0, 1), F), (R, W, 1))
        f["depth"] = np.full((R, W), 5, F)
        f["albedo"] = np.full((R, W, 3), 0.5, F)
        f["samples"] = np.full((R, W), f["spp"], np.int32)
        return f

    # NaN and +-inf colours at a centre and as neighbours: a NaN or inf neighbour has e = NaN or inf, so w is NaN or 0 and
    # never enters; the pixel itself stays NaN (or inf * w0 / w0)
    f = base(1)
    f["accum"][4, 5] = NAN
    f["accum"][1, 1] = INF
    f["accum"][7, 2] = -INF
    f["accum"][2, 8, 1] = NAN
    f["accum"][6, 9] = (INF, -INF, 0)
    f["accum"][0, 0, 2] = INF
    out["nonfinite_colours"] = (f, dict(color_scale=2.0, depth_scale=1.0, normal_squarings=1))
    out["nonfinite_colours_color_scale_zero"] = (f, dict(color_scale=0.0, depth_scale=1.0, normal_squarings=1))
    # subnormal colours: sums, products and quotients stay subnormal (flushed to zero they change)
    f = base(2)
    f["accum"] = (f["accum"] * F(1e-39)).astype(F)
    f["accum"][3, 3] = (1e-45, 0, 3e-45)
    out["subnormal_colours"] = (f, dict(color_scale=1.0, depth_scale=1.0))
    # subnormal weights: e = 1e4, e * e * 1e30 = 1e38, w = H / 1e38 subnormal at k = 0; at k = 1 the product is inf, w = 0
    f = base(3)
    f["accum"] = np.where(np.arange(W)[None, :, None] % 2 == 0, F(0), F(1e4 / 3)) + np.zeros((R, W, 3), F)
    f["accum"][4, 4] = (5, 6, 7)
    out["subnormal_weights"] = (f, dict(color_scale=1e30, depth_scale=1.0))
    # depth weights that go subnormal: dz = 1e19, dz * dz = 1e38
    f = base(4)
    f["depth"] = np.where(np.arange(R)[:, None] % 3 == 0, F(1), F(1e19)) + np.zeros((R, W), F)
    out["subnormal_depth_weights"] = (f, dict(color_scale=0.0, depth_scale=1.0))
    # albedo at, just below and just above the floor, NaN, zero and negative, component by component
    f = base(5)
    floor = F(0.25)
    vals = [floor, _ulps(floor, -1), _ulps(floor, 1), NAN, F(0), F(-1), INF, F(1e-40)]
    for idx, v in enumerate(vals):
        f["albedo"][idx % R, (3 * idx) % W, idx % 3] = v
        f["albedo"][(idx + 4) % R, (2 * idx + 1) % W] = v
    out["albedo_floor"] = (f, dict(color_scale=1.0, depth_scale=0.5, albedo_floor=0.25, flags=DEMODULATE))
    out["albedo_floor_zero"] = (f, dict(color_scale=1.0, depth_scale=0.5, albedo_floor=0.0, flags=DEMODULATE))
    # sample counts 0, 1, negative and above spp
    f = base(6)
    f["samples"] = np.random.RandomState(6).choice(np.array([0, 1, 12, 5, -3, 40], np.int32), (R, W)).astype(np.int32)
    out["samples"] = (f, dict(color_scale=1.0, depth_scale=1.0))
    # normals orthogonal, opposite and zero, beside one another; a miss (999999) beside finite depths
    f = base(7)
    f["normal"][:, 4:7] = (1, 0, 0)
    f["normal"][:, 7:] = (0, 0, -1)
    f["normal"][3:6, 1:3] = 0
    f["depth"][3:6, 1:3] = MISS_DEPTH
    f["normal"][8, 10] = (NAN, 0, 1)
    f["depth"][0, 5] = NAN
    f["depth"][0, 9] = INF
    for sq in (0, 1, 8):
        out[f"normals_squarings{sq}"] = (f, dict(color_scale=0.5, depth_scale=1.0, normal_squarings=sq))
    # normals a little off unit length and off parallel: t in (0, 1) and above 1, squared up to 8 times (underflow, overflow)
    f = base(8)
    r = np.random.RandomState(8)
    f["normal"] = (f["normal"] * (1 + 0.2 * (r.rand(R, W, 1) - 0.5)) + 0.3 * (r.rand(R, W, 3) - 0.5)).astype(F)
    f["normal"][2, 2] = (0, 0, 1.5)
    f["normal"][2, 3] = (0, 0, 1.4)
    out["normals_off_unit_squarings8"] = (f, dict(color_scale=0.5, depth_scale=1.0, normal_squarings=8))
    for f, _ in out.values():
        for a in f.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def two_regions(seed, width=24, rows=20):
    """A frame of two regions with orthogonal normals (left: +z, right: +x) and finite colours: (frame, left mask)."""
    f = random_frame(seed, width, rows)
    left = np.zeros((rows, width), bool)
    left[:, : width // 2 + 1] = True
    left[rows // 2:, : width // 3] = False  # (a border that is not a straight line)
    f["normal"] = np.where(left[..., None], np.array((0, 0, 1), F), np.array((1, 0, 0), F)).astype(F)
    f["depth"] = np.where(left, F(3), F(4)).astype(F)
    return f, left


def noise_frame(seed=20240921, size=128, level=0.5, sigma=0.1):
    """iid noise on a constant image, for the variance property: float32 [size, size, 3]"""
    r = np.random.RandomState(seed)
    return (level + sigma * r.randn(size, size, 3)).astype(F)
