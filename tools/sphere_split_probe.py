#!/usr/bin/env python
"""Pipelined frame time of a sphere scene on one route (not bench.py's workload).

  python tools/sphere_split_probe.py --scene open5 --route split [--width 1920 --height 1080 --spp 64 --frames 200]

Renders `--frames` pipelined frames (DeviceScene.frame_loop: RTC_F_OVERLAP launches, SDMA copies into pinned host
buffers) after a warm-up loop and prints one JSON line with the loop's wall time (RtcLoopStats.wallMs) per frame.

  --route auto    the upload gate decides (rtc_scene_sphere_split)
  --route split   RTC_F_SPLIT_SPHERES: tile cull with sphere coverage + sky pass + rtc_render_chain<SPHERES>
  --route nocoop  RTC_F_NO_COOP: the one-lane-per-pixel kernel

`auto` and `nocoop` use only what older builds of librtc.so export, so RTC_LIB_PATH=<an older librtc.so> times that build
with the same script (its `auto` is the one-lane-per-pixel kernel for every scene with spheres).

Scenes: default (the reference's closed box and sphere, scene.h), open5 (ultracomplex + five spheres, open), open5_closed
(open5 inside a sphere of radius 50), spheres_only (open5's spheres, no triangle).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def scene_of(name):
    from conftest import load_tris, scene_spheres
    from sphere_scenes import closing_sphere, open5

    if name == "default":
        return load_tris("default")[0], scene_spheres("default")
    if name == "open5":
        return load_tris("ultracomplex")[0], open5()
    if name == "open5_closed":
        return load_tris("ultracomplex")[0], np.concatenate([open5(), closing_sphere(50.0, (0.0, 0.0, 0.0))])
    if name == "spheres_only":
        return None, open5()
    raise SystemExit(f"unknown scene {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="open5")
    ap.add_argument("--route", choices=["auto", "split", "nocoop"], default="auto")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--buffers", type=int, default=3)
    a = ap.parse_args()

    import torch

    import raytracingc_amd as rt

    tris, sph = scene_of(a.scene)
    scene, cam = rt.default_scene(), rt.camera_basis()
    kw = {}
    if a.route == "split":
        kw["split_spheres"] = True
    cfg = rt.RenderConfig(a.width, a.height, a.spp, 10, False, coop=a.route != "nocoop", **kw)
    ds = rt.DeviceScene(tris, sph)
    new_api = hasattr(rt.lib(), "rtc_scene_sphere_split")
    st = torch.cuda.Stream()
    dev = [torch.zeros((a.height, a.width, 3), dtype=torch.uint8, device="cuda") for _ in range(a.buffers)]
    host = [torch.zeros((a.height, a.width, 3), dtype=torch.uint8, pin_memory=True) for _ in range(a.buffers)]
    torch.cuda.synchronize()
    args = (scene, cam, cfg, [d.data_ptr() for d in dev], [h.data_ptr() for h in host], a.width * 3)
    ds.frame_loop(*args, a.warmup, st.cuda_stream)
    out = ds.frame_loop(*args, a.frames, st.cuda_stream)
    print(json.dumps({
        "scene": a.scene, "route": a.route, "lib": os.environ.get("RTC_LIB_PATH") or "tree",
        "width": a.width, "height": a.height, "spp": a.spp, "frames": out["frames"],
        "wall_ms": round(out["wall_ms"], 4), "ms_per_frame": round(out["wall_ms"] / out["frames"], 5),
        "hit_share_all": float(rt.bounce_hit_share(tris, sph)) if new_api else None,
        "sphere_split": ds.sphere_split if new_api else None,
        "checksum": int(host[0].numpy().astype(np.uint64).sum()),
    }), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
