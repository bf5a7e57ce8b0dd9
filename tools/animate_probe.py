#!/usr/bin/env python
"""What moving geometry costs per pipelined frame (not bench.py's workload), on one device.

  python tools/animate_probe.py [--scene ultracomplex --width 1920 --height 1080 --spp 64 --frames 40 --rounds 7
                                 --upload-frames 5 --out profiles/NAME.json]

Variants, each `--frames` overlapped whole frames (RTC_F_OVERLAP) on one stream into two alternating Color buffers:
  frames          no update: the static scene's pipelined period
  translate       before each frame the triangles (a float32 [n, 17] device tensor) are translated a little on the device
                  by a torch kernel on the launch stream, and nothing reads them: the producer's own cost
  reprepare       no update, but two cameras alternate whose origins differ by 1e-6: every frame derives its primary
                  records again (rtc_prep_primary), as every frame after an update must
  update          the same translation, then DeviceScene.update(tris=tensor) (rtc_scene_update_async), then the frame
  upload          the only alternative without an update: rtc_scene_release + rtc_scene_upload of host triangles before
                  each frame (two host arrays alternate; `--upload-frames` frames, it is slow)
and `refit_us`: the refit kernel alone, device time of 50 updates back to back between two events, per update.

After a warm-up of every variant, `--rounds` rounds run the variants one after the other (alternated, so that drift and
other tenants of the machine hit all alike); a round is timed by the host clock around its frames, ending in a device
synchronise.  Printed (one JSON line, also written to --out): per variant the median, minimum and maximum ms per frame
over the rounds, and update - translate, update - frames and reprepare - frames in microseconds from the medians.  The
translation moves the triangles by +d on even frames and -d on odd ones, so the geometry stays where the upload clustered
it; after the timed rounds the probe checks that the updated scene's frame equals a fresh upload's of the same triangles,
byte for byte."""
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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--upload-frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from conftest import load_tris

    import raytracingc_amd as rt

    tris, _ = load_tris(a.scene)
    scene, cam = rt.default_scene(), rt.camera_basis()
    cfg = rt.RenderConfig(a.width, a.height, a.spp, 10, True, overlap=True)
    state = {"ds": rt.DeviceScene(tris, None), "k": 0}
    bufs = [torch.zeros((a.height, a.width, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    dev = torch.from_numpy(tris.copy().view(np.float32).reshape(len(tris), 17)).cuda()
    delta = torch.tensor([0.01, -0.005, 0.0075] * 3, dtype=torch.float32, device="cuda")
    moved = tris.copy()
    for v in ("posA", "posB", "posC"):
        for c, d in zip("xyz", (0.01, -0.005, 0.0075)):
            moved[v][c] = moved[v][c] + np.float32(d)
    hosts = [tris, moved]
    torch.cuda.synchronize()

    cam2 = rt.camera_basis((rt.DEFAULT_ORIGIN[0] + 1e-6, rt.DEFAULT_ORIGIN[1], rt.DEFAULT_ORIGIN[2]))

    def frame(camera=cam):
        state["ds"].render_rows_async(scene, camera, cfg, bufs[state["k"] % 2].data_ptr(), stream=st)
        state["k"] += 1

    def v_reprepare():
        frame(cam2 if state["k"] % 2 else cam)

    def translate():
        with torch.cuda.stream(stream):
            dev[:, :9].add_(delta if state["k"] % 2 == 0 else -delta)

    def v_translate():
        translate()
        frame()

    def v_update():
        translate()
        state["ds"].update(tris=dev, stream=st)
        frame()

    def v_upload():
        torch.cuda.synchronize()  # (release drains the scene's streams anyway)
        state["ds"].close()
        state["ds"] = rt.DeviceScene(hosts[state["k"] % 2], None)
        frame()

    variants = {"frames": (frame, a.frames), "translate": (v_translate, a.frames),
                "reprepare": (v_reprepare, a.frames), "update": (v_update, a.frames),
                "upload": (v_upload, a.upload_frames)}
    ms = {k: [] for k in variants}
    for fn, _ in variants.values():  # warm-up
        fn()
        fn()
        torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (fn, n) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / n)
    # the refit kernel alone
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    for _ in range(50):
        state["ds"].update(tris=dev, stream=st)
    e1.record(stream)
    torch.cuda.synchronize()
    refit_us = e0.elapsed_time(e1) * 1e3 / 50
    # the updated scene renders what a fresh upload of the same triangles renders
    state["ds"].update(tris=dev, stream=st)
    frame()
    torch.cuda.synchronize()
    got = bufs[(state["k"] - 1) % 2].cpu()
    now = dev.cpu().numpy().reshape(-1).view(rt.TRIANGLE_DT)
    want, _, _ = rt.render(now, None, scene, cam, rt.RenderConfig(a.width, a.height, a.spp, 10, True))
    if not np.array_equal(got.numpy(), want):
        raise SystemExit("the updated scene's frame differs from a fresh upload's")
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"scene": a.scene, "triangles": len(tris), "width": a.width, "height": a.height, "spp": a.spp,
           "frames": a.frames, "upload_frames": a.upload_frames, "rounds": a.rounds,
           "ms_per_frame": {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                            for k, v in ms.items()},
           "refit_us": round(refit_us, 3),
           "update_minus_translate_us": round((med["update"] - med["translate"]) * 1e3, 3),
           "update_minus_frames_us": round((med["update"] - med["frames"]) * 1e3, 3),
           "reprepare_minus_frames_us": round((med["reprepare"] - med["frames"]) * 1e3, 3),
           "upload_over_update": round(med["upload"] / med["update"], 1)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    state["ds"].close()


if __name__ == "__main__":
    main()
