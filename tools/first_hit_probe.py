#!/usr/bin/env python
"""Device time of the first-hit launch (rtc_render_first_hit_async) beside the cheapest render launch that
traces the same rays, and a pipelined frame loop with and without one first-hit launch per frame.  Not bench.py's workload.

  python tools/first_hit_probe.py [--scene ultracomplex] [--sizes 1920x1080,3840x2160] [--launches 30] [--rounds 3]
                                  [--loop-frames 200]

Per size, four launches on one stream, each between two HIP events (torch.cuda.Event), after a warm-up of every one:
  all4      the first-hit launch with prim, depth, normal and albedo
  prim      ... with prim alone
  brute     ... with all four and RTC_F_NO_TILE_CULL
  render1   rtc_render_rows_async with spp = 1, maxBounce = 1 (joined): the same primary segment plus the environment
            and 3 B of Color per pixel -- what a caller had before this launch existed
The four alternate launch by launch, `--launches` times per round; a round's figure is the median of its launches, and
the rounds' medians with their spread (max - min over the rounds) are printed: a difference inside the spread is none.
The loop: `--loop-frames` RTC_F_OVERLAP frames of 1920x1080x64 enqueued back to back on one stream (tools/frame_loop.py's
loop), the wall time per frame from a host clock around the loop and a device synchronise, alternately without and with
one first-hit launch (all four buffers) after every frame.  One JSON line per measurement."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="ultracomplex")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-frames", type=int, default=200)
    a = ap.parse_args()
    if a.launches < 20:
        raise SystemExit("at least 20 launches per round")

    import torch

    import raytracingc_amd as rt
    from conftest import load_tris

    if rt.device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    tris, _ = load_tris(a.scene)
    ds = rt.DeviceScene(tris, None)
    scene, cam = rt.default_scene(), rt.camera_basis()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream

    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        prim = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        normal = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        albedo = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        colors = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        hit, brute = rt.RenderConfig(W, H, 0, 0, True), rt.RenderConfig(W, H, 0, 0, True, tile_cull=False)
        one = rt.RenderConfig(W, H, 1, 1, True)
        four = dict(prim_ptr=prim.data_ptr(), depth_ptr=depth.data_ptr(), normal_ptr=normal.data_ptr(),
                    albedo_ptr=albedo.data_ptr())
        launches = {
            "all4": lambda: ds.render_first_hit_async(cam, hit, stream=sp, **four),
            "prim": lambda: ds.render_first_hit_async(cam, hit, prim_ptr=prim.data_ptr(), stream=sp),
            "brute": lambda: ds.render_first_hit_async(cam, brute, stream=sp, **four),
            "render1": lambda: ds.render_rows_async(scene, cam, one, colors.data_ptr(), None, None, sp),
        }
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
        base = statistics.median(medians["render1"])
        for k, m in medians.items():
            print(json.dumps({"what": "launch", "scene": a.scene, "size": size, "launch": k, "launches_per_round": a.launches,
                              "round_medians_ms": [round(v, 4) for v in m], "median_ms": round(statistics.median(m), 4),
                              "spread_ms": round(max(m) - min(m), 4),
                              "vs_render1": round(statistics.median(m) / base, 3)}), flush=True)
        hits = int((prim >= 0).sum().item())
        print(json.dumps({"what": "check", "size": size, "hit_pixels": hits, "pixels": W * H}), flush=True)

    if a.loop_frames > 0:
        W, H = 1920, 1080
        cfg = rt.RenderConfig(W, H, 64, 10, True, overlap=True)
        hit = rt.RenderConfig(W, H, 0, 0, True)
        bufs = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
        prim = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        normal = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        albedo = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")

        def loop(frames, with_hit):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(frames):
                ds.render_rows_async(scene, cam, cfg, bufs[f % 3].data_ptr(), None, None, sp)
                if with_hit:
                    ds.render_first_hit_async(cam, hit, prim.data_ptr(), depth.data_ptr(), normal.data_ptr(),
                                              albedo.data_ptr(), sp)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / frames

        loop(20, False), loop(20, True)
        res = {False: [], True: []}
        for _ in range(a.rounds):
            for with_hit in (False, True):
                res[with_hit].append(loop(a.loop_frames, with_hit))
        for with_hit, m in res.items():
            print(json.dumps({"what": "loop", "scene": a.scene, "size": "1920x1080x64", "first_hit_per_frame": with_hit,
                              "frames": a.loop_frames, "round_ms_per_frame": [round(v, 4) for v in m],
                              "median_ms_per_frame": round(statistics.median(m), 4),
                              "spread_ms": round(max(m) - min(m), 4)}), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
