#!/usr/bin/env python
"""Device time of the occlusion query (rtc_occluded_async) beside the existing way to the same answer
(rtc_trace_rays_async with the depth buffer only, compared with the limit afterwards), on two ray sets, coherent and
incoherent, with and without the ball cull.  Not bench.py's workload.

  python tools/occluded_probe.py [--scene ultracomplex] [--size 1920x1080] [--launches 30] [--rounds 3]

Ray sets, each in raster order and in one fixed random permutation (rays and limits together):
  A      the primary rays of the golden camera's frame (tests/primary_rays.launch_rays: 2,073,600 at 1080p), no limit
  B2     ambient-occlusion rays: origins at the first-hit points of A's rays that hit, one direction per point around the
         stored normal (normalized(normal + a unit vector drawn with a fixed seed)), tMax = 2 % of the scene's bounding-box
         diagonal
  B20    the same rays with tMax = 20 % of the diagonal
Per set and order, four launches on one stream, each between two HIP events (torch.cuda.Event), after a warm-up of all:
  occ        flags 0: the ball cull, bytes and count out
  brute      RTC_F_NO_CLUSTER_CULL
  bytes      flags 0 with the bytes only (no counter: what the one atomic add per wave costs)
  closest    rtc_trace_rays_async, flags 0, the depth buffer only
They alternate launch by launch, `--launches` times per round; a round's figure is the median of its launches, and the
rounds' medians with their spread (max - min over the rounds) are printed: a difference inside the spread is none.  Before
anything is timed every flag variant's bytes and count are compared with depth < tMax (and depth < 999999) of the closest
launch on the same rays.  One JSON line per measurement."""
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
    ap.add_argument("--warmup", type=int, default=3)
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
    host = launch_rays(cam, rt.RenderConfig(W, H, 0, 0, True)).view(np.float32).reshape(-1, 6)
    verts = np.stack([np.stack([tris[p][c] for c in "xyz"], -1) for p in ("posA", "posB", "posC")]).reshape(-1, 3)
    diagonal = float(np.linalg.norm(verts.max(0).astype(np.float64) - verts.min(0).astype(np.float64)))
    st = torch.cuda.current_stream()
    sp = st.cuda_stream

    # the AO rays from the first hits of A (on the device: the query's own buffers)
    primary = torch.from_numpy(host.copy()).cuda()
    first = ds.trace_rays(primary, True, ("prim", "depth", "normal"))
    hit = first["prim"] >= 0
    point = host[hit, 0:3] + host[hit, 3:6] * first["depth"][hit, None]
    rnd = np.random.default_rng(7).normal(size=(int(hit.sum()), 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    dirs = first["normal"][hit].astype(np.float64) + rnd
    dirs /= np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-12)
    ao = np.concatenate([point, dirs], 1).astype(np.float32)

    sets = {}
    for name, rays, lim in (("A", host, None), ("B2", ao, 0.02 * diagonal), ("B20", ao, 0.20 * diagonal)):
        n = len(rays)
        perm = np.random.default_rng(2024).permutation(n)
        for order, idx in (("raster", np.arange(n)), ("permuted", perm)):
            sets[f"{name}_{order}"] = {
                "n": n, "rays": torch.from_numpy(rays[idx].copy()).cuda(),
                "tmax": None if lim is None else torch.full((n,), lim, dtype=torch.float32, device="cuda"), "limit": lim}
    nmax = max(s["n"] for s in sets.values())
    occ = torch.zeros(nmax, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    depth = torch.zeros(nmax, dtype=torch.float32, device="cuda")
    flags = {"occ": 0, "brute": rt.RTC_F_NO_CLUSTER_CULL}

    def launch(s, kind):
        if kind == "closest":
            return lambda: ds.trace_rays_async(s["rays"].data_ptr(), s["n"], True, 0, depth_ptr=depth.data_ptr(), stream=sp)
        tmax = s["tmax"].data_ptr() if s["tmax"] is not None else 0
        if kind == "bytes":  # flags 0 without the counter: what the one atomic per wave costs
            return lambda: ds.occluded_async(s["rays"].data_ptr(), s["n"], tmax, True, 0, occ.data_ptr(), 0, stream=sp)
        return lambda: ds.occluded_async(s["rays"].data_ptr(), s["n"], tmax, True, flags[kind], occ.data_ptr(),
                                         cnt.data_ptr(), stream=sp)

    launches = {f"{sn}_{kind}": launch(s, kind) for sn, s in sets.items() for kind in (*flags, "bytes", "closest")}
    # every flag variant agrees with the closest-hit launch's depth < tMax before anything is timed
    for sn, s in sets.items():
        launches[f"{sn}_closest"]()
        torch.cuda.synchronize()
        d = depth[:s["n"]]
        want = (d < 999999.0) if s["tmax"] is None else ((d < s["tmax"]) & (d < 999999.0))
        for kind in flags:
            occ.zero_()
            cnt.zero_()
            launches[f"{sn}_{kind}"]()
            torch.cuda.synchronize()
            same = bool(torch.equal(occ[:s["n"]].bool(), want)) and int(cnt.item()) == int(want.sum().item())
            print(json.dumps({"what": "check", "set": sn, "launch": kind, "equals_depth_below_tmax": same, "rays": s["n"],
                              "tmax": s["limit"], "occluded": int(want.sum().item())}), flush=True)
            if not same:
                raise SystemExit("the occlusion query and the closest-hit launch disagree")
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
        sn = k.rsplit("_", 1)[0]
        n = sets[sn]["n"]
        print(json.dumps({"what": "launch", "scene": a.scene, "triangles": len(tris), "size": a.size, "diagonal": round(diagonal, 3),
                          "set": sn, "launch": k[len(sn) + 1:], "rays": n, "tmax": sets[sn]["limit"],
                          "launches_per_round": a.launches, "round_medians_ms": [round(v, 4) for v in m],
                          "median_ms": round(statistics.median(m), 4), "spread_ms": round(max(m) - min(m), 4),
                          "ns_per_ray": round(statistics.median(m) * 1e6 / n, 3)}), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
