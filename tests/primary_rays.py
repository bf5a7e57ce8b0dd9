"""The primary rays of a launch, restated in numpy float32 (main.c:88-93 with moremath.c:7-17's operation order), and the
reference's verdict on every (pixel, triangle) pair of a launch through the CPU oracle.  Shared by
tests/test_gpu_item_records.py (the item records carry exactly these bits), tests/test_adversarial_scenes.py and
tests/test_gpu_primary_cull.py."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

from raytracingc_amd._abi import RAY_DT, TRIANGLE_DT

# calculateRayCollision's initial closest distance (raytracing.c:218): a rayTriangle hit is recorded only below it
NO_HIT_DST = np.float32(999999)


def launch_rows(cfg):
    """Image row of every launch row (rtc.h: y = rowStart + k*rowStride, or bands of rowBand rows)."""
    B = max(cfg.row_band, 1)
    r = np.arange(cfg.rows())
    return cfg.row_start + (r // B) * cfg.row_stride * B + r % B


def primary_dirs(cam, cfg, x, y):
    """main.c:88-93 for the pixels (x, y), float32 operation by operation: integer halves, int -> float, f32 divides,
    plus(plus(times(ex, dx), times(ey, dy)), times(ez, fov)), then normalized (moremath.c:7-17: the f32 sum of squares left
    to right, sqrt and 1./length in double, each rounded to float, three f32 products)."""
    f = np.float32
    v = lambda a: np.array([a.x, a.y, a.z], f)  # noqa: E731
    W, H = cfg.width, cfg.height
    with np.errstate(all="ignore"):
        dx = ((x - W // 2).astype(f) / f(H // 2))[:, None]
        dy = ((y - H // 2).astype(f) / f(H // 2))[:, None]
        d = (((v(cam.ex) * dx).astype(f) + (v(cam.ey) * dy).astype(f)).astype(f) + (v(cam.ez) * f(cam.fov)).astype(f)).astype(f)
        sq = (d * d).astype(f)
        ss = ((sq[:, 0] + sq[:, 1]).astype(f) + sq[:, 2]).astype(f)
        length = np.sqrt(ss.astype(np.float64)).astype(f)
        inv = (1.0 / length.astype(np.float64)).astype(f)
        return (d * inv[:, None]).astype(f)


def launch_rays(cam, cfg):
    """Ray[] of every pixel of the launch, launch row by launch row (pixel r * width + x)."""
    rows = launch_rows(cfg)
    x = np.tile(np.arange(cfg.width), len(rows))
    y = np.repeat(rows, cfg.width)
    d = primary_dirs(cam, cfg, x, y)
    rays = np.zeros(len(x), RAY_DT)
    for k, c in enumerate("xyz"):
        rays["pos"][c] = np.float32(getattr(cam.origin, c))
        rays["dir"][c] = d[:, k]
    return rays


def hit_table(oracle_ray_triangle, tris, rays, threads=8):
    """rayTriangle (the oracle's) for every ray against every triangle: (recorded bool [rays, triangles], dst float32
    [rays, triangles]).  recorded = didHit and dst < 999999: what calculateRayCollision can take as the closest hit
    (raytracing.c:218-231; a NaN dst, which rayTriangle reports as a hit since every comparison with NaN is false, is never
    below the running closest distance)."""
    tris = np.ascontiguousarray(tris, TRIANGLE_DT)
    n = len(rays)

    def one(t):
        hit, dst = oracle_ray_triangle(rays, np.repeat(tris[t:t + 1], n))
        return hit != 0, dst

    with ThreadPoolExecutor(threads) as ex:
        cols = list(ex.map(one, range(len(tris))))
    hit = np.stack([c[0] for c in cols], 1)
    dst = np.stack([c[1] for c in cols], 1)
    with np.errstate(invalid="ignore"):
        return hit & (dst < NO_HIT_DST), dst


def _round_dir(x, up):
    """The float32 next to the double x in the given direction (__double2float_ru / _rd)."""
    with np.errstate(all="ignore"):
        f = x.astype(np.float32)
        wrong = (f.astype(np.float64) < x) if up else (f.astype(np.float64) > x)
        return np.where(wrong, np.nextafter(f, np.float32(np.inf if up else -np.inf)), f).astype(np.float32)


def prep_records(tris, origin):
    """rtc_prep_primary restated (rtc_closest.h): per triangle the float32 AB, AC, s0 = origin - A,
    q0 = s0 x AB and dAC0 = dot(AC, q0) as the kernel forms them, its error terms in double with the proof's constants
    (9.006 u, 6.002 u, 2.0002 u, 4.8e-7, the factor 4, 2^-60) and its two escape hatches: `sane` (ed < 2.5e-4, products below
    1e30) and `never` (dAC0 is 0 or NaN).  Returns a dict with sane, never, ed and rec float32 [n, 16], the DevPrimF
    records {N, mnd, sigma Gd, c, sigma Gu, -m, sigma q0, 0} with the margins rounded outwards."""
    f = np.float32
    g = lambda k: np.stack([tris[k][c] for c in "xyz"], 1).astype(f)  # noqa: E731
    o = np.array([origin.x, origin.y, origin.z], f)
    with np.errstate(all="ignore"):
        A, N = g("posA"), g("normal")
        AB, AC, s0 = (g("posB") - A).astype(f), (g("posC") - A).astype(f), (o[None, :] - A).astype(f)

        def cross(u, v, t):  # each product and each difference rounded to t
            return np.stack([((u[:, 1] * v[:, 2]).astype(t) - (u[:, 2] * v[:, 1]).astype(t)).astype(t),
                             ((u[:, 2] * v[:, 0]).astype(t) - (u[:, 0] * v[:, 2]).astype(t)).astype(t),
                             ((u[:, 0] * v[:, 1]).astype(t) - (u[:, 1] * v[:, 0]).astype(t)).astype(t)], 1)

        q0 = cross(s0, AB, f)
        p = (AC * q0).astype(f)
        dac0 = ((p[:, 0] + p[:, 1]).astype(f) + p[:, 2]).astype(f)
        d = np.float64
        gd, gu = cross(AC.astype(d), AB.astype(d), d), cross(AC.astype(d), s0.astype(d), d)
        n1 = lambda a: (np.abs(a[:, 0].astype(d)) + np.abs(a[:, 1].astype(d))) + np.abs(a[:, 2].astype(d))  # noqa: E731
        u = 2.0 ** -24
        nAB, nAC, nS, nQ, nN = n1(AB), n1(AC), n1(s0), n1(q0), n1(N)
        eD, eU, eV = 9.006 * u * nAB * nAC, 9.006 * u * nS * nAC, 6.002 * u * nQ
        eW = eD + eU + eV + 2.0002 * u * (nAB * nAC + nS * nAC + nQ) + 4.8e-7 * nAB * nAC
        m = np.maximum(np.maximum(eU, eV), eW) * 4.0 + 2.0 ** -60
        ed, mnd = eD * 4.0, 6.002 * u * nN * 4.0
        sane = (ed < 2.5e-4) & (nAB * nAC < 1e30) & (nS * nAC < 1e30) & (nQ < 1e30) & (m < 1e30) & (mnd < 1e30)
        never = ~((dac0 < 0) | (dac0 > 0))
        sg = np.where(dac0 < 0, f(-1), f(1))[:, None]
        zero, inf = np.zeros(len(tris), f), np.full(len(tris), np.inf, f)
        vec = lambda v: np.where(sane[:, None], (sg * v.astype(f)).astype(f), f(0))  # noqa: E731
        rec = np.zeros((len(tris), 16), f)
        rec[:, 0:3] = N
        rec[:, 3] = np.where(never, -inf, np.where(sane, _round_dir(mnd, True), inf))
        rec[:, 4:7] = vec(gd)
        rec[:, 7] = np.where(sane, _round_dir(d(f(0.001)) - ed, False), -inf)
        rec[:, 8:11] = vec(gu)
        rec[:, 11] = np.where(sane, -_round_dir(m, True), -inf)
        rec[:, 12:15] = vec(q0)
        rec[:, 15] = zero
    return {"sane": sane, "never": never, "ed": ed, "rec": rec}


def prep_flags(tris, origin):
    """(sane, never, ed) of prep_records."""
    r = prep_records(tris, origin)
    return r["sane"], r["never"], r["ed"]


def tile_cones(cam, cfg, tiles_x, tiles):
    """rect_cone (rtc_layout.h) restated in double for every 8x8 tile of the launch: float64 [tiles, 4] =
    {eDir = 16 u S / vmin + 4 u, vmin, vmax, usable}."""
    f, d = np.float32, np.float64
    W, H, rows = cfg.width, cfg.height, cfg.rows()
    B = max(cfg.row_band, 1)
    row_y = lambda r: cfg.row_start + (r // B) * cfg.row_stride * B + r % B  # noqa: E731
    v3 = lambda a: np.array([a.x, a.y, a.z], f)  # noqa: E731
    ex, ey, ez, fov = v3(cam.ex).astype(d), v3(cam.ey).astype(d), v3(cam.ez).astype(d), d(f(cam.fov))
    ezl = np.sqrt((ez[0] * ez[0] + ez[1] * ez[1]) + ez[2] * ez[2])
    unit = bool((np.abs(np.concatenate([v3(cam.ex), v3(cam.ey), v3(cam.ez)])) <= f(1.0001)).all())
    u = 2.0 ** -24
    out = np.zeros((tiles, 4), d)
    with np.errstate(all="ignore"):
        for t in range(tiles):
            tx, ty = t % tiles_x, t // tiles_x
            x0, x1, r0, r1 = tx * 8, min(tx * 8 + 7, W - 1), ty * 8, min(ty * 8 + 7, rows - 1)
            dxs = [d(f(x - W // 2) / f(H // 2)) for x in (x0, x1)]
            dys = [d(f(row_y(r) - H // 2) / f(H // 2)) for r in (r0, r1)]
            vmin, vmax, finite = 1e300, 0.0, bool(0.0 < ezl < 1e300)
            for k in range(4):
                dx, dy = dxs[k & 1], dys[k >> 1]
                v = (ex * dx + ey * dy) + ez * fov
                finite = finite and bool(np.isfinite(v).all())
                vmax = max(vmax, np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
                vmin = min(vmin, ((v[0] * ez[0] + v[1] * ez[1]) + v[2] * ez[2]) / ezl)
            S = (max(abs(dxs[0]), abs(dxs[1])) + max(abs(dys[0]), abs(dys[1]))) + abs(fov)
            kmin, kmax = vmin * (1.0 - 1e-12), vmax * (1.0 + 1e-12)
            e_dir = 16.0 * u * S / kmin + 4.0 * u
            ok = finite and unit and kmin > 1e-6 and e_dir < 1e-3 and np.isfinite(S)
            out[t] = (e_dir, kmin, kmax, 1.0 if ok else 0.0)
    return out
