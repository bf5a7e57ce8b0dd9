#!/usr/bin/env python
"""Device time of the three ray queries on permuted rays with and without the ray order (rtc_ray_order_async, rtc_gather_async,
rtc_scatter_async), under tools/trace_paths_probe.py's protocol: HIP events on one stream, the launches
alternated in one process, medians of `--launches` (30) in each of `--rounds` (3) rounds, the spread over the rounds.  Not
bench.py's workload.

  python tools/ray_order_probe.py [--scene ultracomplex] [--size 1920x1080] [--spp 64] [--max-bounce 10]

The rays are the primary rays of the golden camera's frame (2,073,600 at 1080p) with the pixels' seeds, in raster order and in
the fixed permutation of seed 2024.  Legs:
  paths (a) raster, (e) permuted: trace_paths_probe.py's legs of those names; (o) permuted and ordered: order, gather of rays
        and seeds, the query, scatter of radiance and seeds -- timed whole and part by part, and the query alone on rays
        gathered once (a reused order); the same (e) and (o) on the default box with its sphere
  rays  rtc_trace_rays_async (all four buffers), permuted, with and without the order
  occ   rtc_occluded_async without limits, bytes only and bytes with the count, permuted, with and without the order
Before anything is timed every ordered output is compared with the unordered one word for word (NaN for NaN).  The verdict
per pair is the project's bar: the median gain must be at least three times the larger spread.  One JSON line per figure."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="ultracomplex")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--max-bounce", type=int, default=10)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.launches < 20:
        raise SystemExit("at least 20 launches per round")

    import numpy as np
    import torch

    import raytracingc_amd as rt
    from conftest import load_tris, scene_spheres
    from primary_rays import launch_rays

    if rt.device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    W, H = (int(v) for v in a.size.split("x"))
    cam, scene = rt.camera_basis(), rt.default_scene()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream

    def same(x, y):
        x, y = x.reshape(-1), y.reshape(-1)
        if x.dtype != torch.float32:
            return bool((x == y).all().item())
        return bool(((x.view(torch.int32) == y.view(torch.int32)) | (torch.isnan(x) & torch.isnan(y))).all().item())

    def setup(tris, spheres, tonly):
        ds = rt.DeviceScene(tris, spheres)
        host = launch_rays(cam, rt.RenderConfig(W, H, 0, 0, tonly)).view(np.float32).reshape(-1, 6)
        n = len(host)
        seeds = np.arange(n, dtype=np.uint32).view(np.int32)
        perm = np.random.default_rng(2024).permutation(n)
        z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
        b = {"rays": torch.from_numpy(host.copy()).cuda(), "seeds": torch.from_numpy(seeds.copy()).cuda(),
             "rays_p": torch.from_numpy(host[perm].copy()).cuda(), "seeds_p": torch.from_numpy(seeds[perm].copy()).cuda(),
             "order": z(n, dt=torch.int32), "scratch": torch.empty(rt.ray_order_scratch_bytes(n), dtype=torch.uint8, device="cuda"),
             "rays_g": z(n, 6), "seeds_g": z(n, dt=torch.int32),
             "rad": z(n, 3), "rad_g": z(n, 3), "rad_o": z(n, 3), "sd": z(n, dt=torch.int32), "sd_g": z(n, dt=torch.int32),
             "sd_o": z(n, dt=torch.int32),
             "hit": [z(n, dt=torch.int32), z(n), z(n, 3), z(n, 3)], "hit_g": [z(n, dt=torch.int32), z(n), z(n, 3), z(n, 3)],
             "hit_o": [z(n, dt=torch.int32), z(n), z(n, 3), z(n, 3)],
             "occ": z(n, dt=torch.uint8), "occ_g": z(n, dt=torch.uint8), "occ_o": z(n, dt=torch.uint8),
             "cnt": z(1, dt=torch.int64), "cnt_o": z(1, dt=torch.int64)}
        p = lambda k: b[k].data_ptr()  # noqa: E731
        order = lambda: ds.ray_order_async(p("rays_p"), n, p("order"), p("scratch"), b["scratch"].numel(), stream=sp)  # noqa: E731
        g_rays = lambda: rt.gather_async(p("rays_g"), p("rays_p"), p("order"), n, 24, sp)  # noqa: E731

        def paths(rays, seeds, rad, sd):
            return lambda: ds.trace_paths_async(scene, p(rays), p(seeds), n, a.spp, a.max_bounce, p(rad), tonly, 0,
                                                seeds_out_ptr=p(sd), stream=sp)

        def gather_paths():
            g_rays()
            rt.gather_async(p("seeds_g"), p("seeds_p"), p("order"), n, 4, sp)

        def scatter_paths():
            rt.scatter_async(p("rad_o"), p("rad_g"), p("order"), n, 12, sp)
            rt.scatter_async(p("sd_o"), p("sd_g"), p("order"), n, 4, sp)

        def hits(rays, out):
            return lambda: ds.trace_rays_async(p(rays), n, tonly, 0, *(t.data_ptr() for t in b[out]), stream=sp)

        def scatter_hits():
            for src, dst, eb in zip(b["hit_g"], b["hit_o"], (4, 4, 12, 12)):
                rt.scatter_async(dst.data_ptr(), src.data_ptr(), p("order"), n, eb, sp)

        def occ(rays, out, cnt):
            return lambda: ds.occluded_async(p(rays), n, 0, tonly, 0, p(out), p(cnt) if cnt else 0, stream=sp)

        def seq(*fns):
            return lambda: [f() for f in fns]

        q_paths = paths("rays_g", "seeds_g", "rad_g", "sd_g")
        s_occ = lambda: rt.scatter_async(p("occ_o"), p("occ_g"), p("order"), n, 1, sp)  # noqa: E731
        L = {
            "paths a raster": paths("rays", "seeds", "rad", "sd"),
            "paths e permuted": paths("rays_p", "seeds_p", "rad", "sd"),
            "paths o ordered total": seq(order, gather_paths, q_paths, scatter_paths),
            "paths o part order": order, "paths o part gather": gather_paths, "paths o part query": q_paths,
            "paths o part scatter": scatter_paths,
            "rays permuted": hits("rays_p", "hit"),
            "rays ordered total": seq(order, g_rays, hits("rays_g", "hit_g"), scatter_hits),
            "occ bytes permuted": occ("rays_p", "occ", None),
            "occ bytes ordered total": seq(order, g_rays, occ("rays_g", "occ_g", None), s_occ),
            "occ count permuted": occ("rays_p", "occ", "cnt"),
            "occ count ordered total": seq(order, g_rays, occ("rays_g", "occ_g", "cnt_o"), s_occ),
        }
        return ds, n, b, L

    def check(tag, b, L, full):
        """every ordered output against the unordered one, word for word"""
        oks = {}
        L["paths e permuted"]()
        L["paths o ordered total"]()
        torch.cuda.synchronize()
        oks["paths"] = same(b["rad_o"], b["rad"]) and same(b["sd_o"], b["sd"])
        if full:
            L["rays permuted"]()
            L["rays ordered total"]()
            torch.cuda.synchronize()
            oks["rays"] = all(same(x, y) for x, y in zip(b["hit_o"], b["hit"]))
            b["cnt"].zero_(), b["cnt_o"].zero_()
            L["occ count permuted"]()
            L["occ count ordered total"]()
            torch.cuda.synchronize()
            oks["occ"] = same(b["occ_o"], b["occ"]) and int(b["cnt"].item()) == int(b["cnt_o"].item())
        print(json.dumps({"what": "check", "scene": tag, "ordered_equals_unordered": oks}), flush=True)
        if not all(oks.values()):
            raise SystemExit("an ordered query and the unordered one disagree")

    def measure(tag, n, L):
        for _ in range(a.warmup):
            for fn in L.values():
                fn()
        torch.cuda.synchronize()
        med = {k: [] for k in L}
        for _ in range(a.rounds):
            evs = {k: [] for k in L}
            for _ in range(a.launches):
                for k, fn in L.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    evs[k].append((e0, e1))
                torch.cuda.synchronize()
            for k, pairs in evs.items():
                med[k].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs))
        out = {}
        for k, m in med.items():
            out[k] = (statistics.median(m), max(m) - min(m))
            print(json.dumps({"what": "launch", "scene": tag, "size": a.size, "rays": n, "spp": a.spp, "launch": k,
                              "launches_per_round": a.launches, "round_medians_ms": [round(v, 4) for v in m],
                              "median_ms": round(out[k][0], 4), "spread_ms": round(out[k][1], 4)}), flush=True)
        for base, ordered in (("paths e permuted", "paths o ordered total"), ("paths e permuted", "paths o part query"),
                              ("rays permuted", "rays ordered total"), ("occ bytes permuted", "occ bytes ordered total"),
                              ("occ count permuted", "occ count ordered total")):
            if base in out and ordered in out:
                gain, spread = out[base][0] - out[ordered][0], max(out[base][1], out[ordered][1])
                verdict = "order pays" if gain >= 3 * spread else "order loses" if -gain >= 3 * spread else "inside the spread"
                print(json.dumps({"what": "pair", "scene": tag, "unordered": base, "ordered": ordered,
                                  "unordered_ms": round(out[base][0], 4), "ordered_ms": round(out[ordered][0], 4),
                                  "ratio": round(out[base][0] / out[ordered][0], 3), "larger_spread_ms": round(spread, 4),
                                  "verdict": verdict}), flush=True)

    tris, _ = load_tris(a.scene)
    ds, n, b, L = setup(tris, None, True)
    check(a.scene, b, L, True)
    measure(a.scene, n, L)
    ds.close()
    del b, L
    torch.cuda.empty_cache()
    box, _ = load_tris("default")
    bds, bn, bb, BL = setup(box, scene_spheres("default"), False)
    BL = {k: v for k, v in BL.items() if k.startswith("paths") and k != "paths a raster"}
    check("default+sphere", bb, BL, False)
    measure("default+sphere", bn, BL)
    bds.close()


if __name__ == "__main__":
    main()
