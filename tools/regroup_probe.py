#!/usr/bin/env python
"""What a regroup costs and what it buys (not bench.py's workload), on one device.

  python tools/regroup_probe.py [--sizes 1024,4096,... --rounds 5 --width 1920 --height 1080 --spp 64 --frames 12
                                 --out profiles/NAME.json]

Part 1, per scene -- ultracomplex (120 triangles), suzannes (3,868) and random triangles of every size in --sizes: the
device time of one rtc_scene_regroup_async (events around `reps` regroups back to back on one stream, per regroup; the
refit is part of it), of the refit alone (rtc_scene_update_async, likewise) and the wall time of the rtc_scene_upload the
regroup replaces (host clock around the call, which synchronises; the release is outside the window).  Warm-up first, then
--rounds rounds with the three alternated; median, minimum and maximum.  After the timed rounds the regrouped scene's
records are compared with a fresh upload's, byte for byte.  `cap_by_measurement` is the largest power of two among the
sizes up to which, at every size tried, the regroup's median stayed below the upload's.

Part 2, scatter(suzannes) at --width x --height x --spp: a scene uploaded as loaded and updated to the scattered triangles
(stale membership) against the same with a regroup.  Per variant: the pipelined frame (--frames overlapped frames on one
stream, host clock, ms per frame), and trace_rays, trace_paths (4 samples, 4 bounces) and occluded on that frame's primary
rays (device tensors, events, ms per call).  Variants alternate within each round."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def random_tris(n, seed=5):
    """n small triangles at random points of a box in front of the default camera."""
    import numpy as np

    import raytracingc_amd as rt

    rng = np.random.default_rng(seed + n)
    p = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32) + np.float32([0.0, 0.0, 6.0])
    e = rng.uniform(-0.05, 0.05, (2, n, 3)).astype(np.float32)
    t = np.zeros(n, rt.TRIANGLE_DT)
    for k, c in enumerate("xyz"):
        t["posA"][c], t["posB"][c], t["posC"][c] = p[:, k], p[:, k] + e[0][:, k], p[:, k] + e[1][:, k]
    t["normal"]["z"] = -1.0
    t["mat"]["color"]["x"] = t["mat"]["color"]["y"] = t["mat"]["color"]["z"] = 0.7
    return t


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048,4096,8192,16384,32768,65536,131072")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--skip-frames", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from conftest import load_tris
    from moving_scenes import scatter
    from primary_rays import launch_rays

    import raytracingc_amd as rt

    cap = rt.regroup_max_tris()
    stream = torch.cuda.Stream()
    st = stream.cuda_stream

    def dev_of(t):
        d = torch.from_numpy(np.ascontiguousarray(t).copy().view(np.uint8)).cuda()
        torch.cuda.synchronize()
        return d

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # ---- part 1 ----
    scenes = [("ultracomplex", load_tris("ultracomplex")[0]), ("suzannes", load_tris("suzannes")[0])]
    scenes += [(f"random{n}", random_tris(n)) for n in (int(x) for x in a.sizes.split(",") if x) if n <= cap]
    part1 = []
    for name, t in scenes:
        n = len(t)
        moved = scatter(t)
        dev = dev_of(moved)
        ds = rt.DeviceScene(t, None)
        scratch = torch.zeros(ds.regroup_scratch_bytes(), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        reps = 20 if n <= 8192 else 5 if n <= 32768 else 2

        def regroup():
            ds.regroup_async(dev.data_ptr(), None, scratch.data_ptr(), scratch.numel(), st)

        def refit():
            ds.update(tris=dev, stream=st)

        def upload():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh = rt.DeviceScene(moved, None)
            ms = (time.perf_counter() - t0) * 1e3
            fresh.close()
            return ms

        regroup(), refit(), upload()  # warm-up
        torch.cuda.synchronize()
        ms = {"regroup": [], "refit": [], "upload": []}
        for _ in range(a.rounds):
            ms["regroup"].append(timed(regroup, reps))
            ms["refit"].append(timed(refit, reps))
            ms["upload"].append(upload())
        regroup()
        torch.cuda.synchronize()
        got, fresh = ds.records(), rt.DeviceScene(moved, None)
        want = fresh.records()
        fresh.close()
        exact = all(np.array_equal(got[k], want[k]) for k in rt.RECORD_ARRAYS)
        ds.close()
        row = {"scene": name, "triangles": n, "reps": reps, "exact": exact, "ms": {k: stats(v) for k, v in ms.items()}}
        print(json.dumps(row), flush=True)
        part1.append(row)
        if not exact:
            raise SystemExit(f"{name}: the regrouped records differ from a fresh upload's")
    by_measure = 0
    for row in part1:
        if not row["scene"].startswith("random"):
            continue
        if row["ms"]["regroup"]["median"] >= row["ms"]["upload"]["median"]:
            break
        by_measure = row["triangles"]

    # ---- part 2 ----
    part2 = {}
    if not a.skip_frames:
        t0 = load_tris("suzannes")[0]
        t1 = scatter(t0)
        scene, cam = rt.default_scene(), rt.camera_basis()
        cfg = rt.RenderConfig(a.width, a.height, a.spp, 10, True, overlap=True)
        rays_h = launch_rays(cam, rt.RenderConfig(a.width, a.height, 1, 10, True))
        rays = torch.from_numpy(rays_h.view(np.float32).reshape(-1, 6).copy()).cuda()
        nr = rays.shape[0]
        seeds = torch.arange(nr, dtype=torch.int32, device="cuda")
        hit = {k: torch.zeros(s, dtype=d, device="cuda") for k, s, d in
               (("prim", (nr,), torch.int32), ("depth", (nr,), torch.float32))}
        rad = torch.zeros((nr, 3), dtype=torch.float32, device="cuda")
        occ = torch.zeros(nr, dtype=torch.uint8, device="cuda")
        bufs = [torch.zeros((a.height, a.width, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
        handles = {}
        for variant, regroup in (("stale", False), ("regrouped", True)):
            handles[variant] = rt.DeviceScene(t0, None)
            handles[variant].update(t1, regroup=regroup)
        torch.cuda.synchronize()

        def frames(ds):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            for k in range(a.frames):
                ds.render_rows_async(scene, cam, cfg, bufs[k % 2].data_ptr(), stream=st)
            torch.cuda.synchronize()
            return (time.perf_counter() - w0) * 1e3 / a.frames

        def queries(ds):
            return {
                "trace_rays": timed(lambda: ds.trace_rays_async(rays.data_ptr(), nr, True, 0, hit["prim"].data_ptr(),
                                                                hit["depth"].data_ptr(), stream=st), 3),
                "trace_paths": timed(lambda: ds.trace_paths_async(scene, rays.data_ptr(), seeds.data_ptr(), nr, 4, 4,
                                                                  rad.data_ptr(), True, stream=st), 2),
                "occluded": timed(lambda: ds.occluded_async(rays.data_ptr(), nr, 0, True, 0, occ.data_ptr(), stream=st), 3),
            }

        ms = {v: {"frame": [], "trace_rays": [], "trace_paths": [], "occluded": []} for v in handles}
        for v, ds in handles.items():  # warm-up
            frames(ds), queries(ds)
        for _ in range(a.rounds):
            for v, ds in handles.items():
                ms[v]["frame"].append(frames(ds))
                for k, x in queries(ds).items():
                    ms[v][k].append(x)
        # the two render the same frame
        out = {}
        for v, ds in handles.items():
            ds.render_rows_async(scene, cam, cfg, bufs[0].data_ptr(), stream=st)
            torch.cuda.synchronize()
            out[v] = bufs[0].cpu().numpy().copy()
            ds.close()
        if not np.array_equal(out["stale"], out["regrouped"]):
            raise SystemExit("the regrouped scene's frame differs from the stale one's")
        part2 = {"scene": "scatter(suzannes)", "triangles": len(t0), "width": a.width, "height": a.height, "spp": a.spp,
                 "frames": a.frames, "rays": nr, "ms": {v: {k: stats(x) for k, x in d.items()} for v, d in ms.items()}}
        print(json.dumps(part2), flush=True)

    res = {"max_tris": cap, "cap_by_measurement": by_measure, "rounds": a.rounds, "sizes": part1, "scattered": part2}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
