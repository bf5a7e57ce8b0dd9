#!/usr/bin/env python
"""Device time of the ray query (rtc_trace_rays_async) on a frame's worth of rays, with and without the
cluster cull, coherent and incoherent, beside the first-hit launch that answers the same question for camera rays.  Not
bench.py's workload.

  python tools/trace_rays_probe.py [--scene ultracomplex] [--size 1920x1080] [--launches 30] [--rounds 3]

The rays are the primary rays of the golden camera's frame (tests/primary_rays.launch_rays: 2,073,600 at 1080p), four
buffers out.  Six launches on one stream, each between two HIP events (torch.cuda.Event), after a warm-up of every one:
  raster_cull     the rays in raster order, the cluster hierarchy
  raster_brute    ... with RTC_F_NO_CLUSTER_CULL (every record, reference order)
  permuted_cull   the same rays in a fixed random permutation (a wave's 64 rays share nothing but the origin)
  permuted_brute  ... with RTC_F_NO_CLUSTER_CULL
  first_hit       rtc_render_first_hit_async, four buffers: the tile cull's candidates per 8x8 tile
  first_hit_brute ... with RTC_F_NO_TILE_CULL
They alternate launch by launch, `--launches` times per round; a round's figure is the median of its launches, and the
rounds' medians with their spread (max - min over the rounds) are printed: a difference inside the spread is none.  The
buffers of the raster-order query are compared with the first-hit launch's before anything is timed.  One JSON line per
measurement."""
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
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.launches < 20:
        raise SystemExit("at least 20 launches per round")

    import numpy as np
    import torch

    import raytracingc_amd as rt
    from conftest import load_tris
    from primary_rays import launch_rays

    if rt.device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    tris, _ = load_tris(a.scene)
    ds = rt.DeviceScene(tris, None)
    cam = rt.camera_basis()
    W, H = (int(v) for v in a.size.split("x"))
    hit, brute = rt.RenderConfig(W, H, 0, 0, True), rt.RenderConfig(W, H, 0, 0, True, tile_cull=False)
    host = launch_rays(cam, hit).view(np.float32).reshape(-1, 6)
    n = len(host)
    perm = np.random.default_rng(2024).permutation(n)
    raster, permuted = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(host[perm].copy()).cuda()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream

    def buffers():
        return {"prim_ptr": torch.zeros(n, dtype=torch.int32, device="cuda"),
                "depth_ptr": torch.zeros(n, dtype=torch.float32, device="cuda"),
                "normal_ptr": torch.zeros((n, 3), dtype=torch.float32, device="cuda"),
                "albedo_ptr": torch.zeros((n, 3), dtype=torch.float32, device="cuda")}

    q, f = buffers(), buffers()
    qp, fp = {k: v.data_ptr() for k, v in q.items()}, {k: v.data_ptr() for k, v in f.items()}
    no_cull = rt.RTC_F_NO_CLUSTER_CULL
    launches = {
        "raster_cull": lambda: ds.trace_rays_async(raster.data_ptr(), n, True, 0, stream=sp, **qp),
        "raster_brute": lambda: ds.trace_rays_async(raster.data_ptr(), n, True, no_cull, stream=sp, **qp),
        "permuted_cull": lambda: ds.trace_rays_async(permuted.data_ptr(), n, True, 0, stream=sp, **qp),
        "permuted_brute": lambda: ds.trace_rays_async(permuted.data_ptr(), n, True, no_cull, stream=sp, **qp),
        "first_hit": lambda: ds.render_first_hit_async(cam, hit, stream=sp, **fp),
        "first_hit_brute": lambda: ds.render_first_hit_async(cam, brute, stream=sp, **fp),
    }
    # the two ways to the same answer agree before anything is timed
    launches["first_hit"]()
    for name in ("raster_brute", "raster_cull"):
        launches[name]()
        torch.cuda.synchronize()
        same = all(torch.equal(q[k].view(torch.int32).reshape(-1), f[k].view(torch.int32).reshape(-1)) for k in q)
        print(json.dumps({"what": "check", "launch": name, "equals_first_hit": same, "rays": n,
                          "hits": int((q["prim_ptr"] >= 0).sum().item())}), flush=True)
        if not same:
            raise SystemExit("the ray query and the first-hit launch disagree")
    for _ in range(a.warmup):
        for fn in launches.values():
            fn()
    torch.cuda.synchronize()
    medians = {k: [] for k in launches}
    for _ in range(a.rounds):
        evs = {k: [] for k in launches}
        for _ in range(a.launches):
            for k, fn in launches.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                evs[k].append((e0, e1))
        torch.cuda.synchronize()
        for k, pairs in evs.items():
            medians[k].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs))
    for k, m in medians.items():
        print(json.dumps({"what": "launch", "scene": a.scene, "triangles": len(tris), "size": a.size, "rays": n, "launch": k,
                          "launches_per_round": a.launches, "round_medians_ms": [round(v, 4) for v in m],
                          "median_ms": round(statistics.median(m), 4), "spread_ms": round(max(m) - min(m), 4),
                          "ns_per_ray": round(statistics.median(m) * 1e6 / n, 3)}), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
