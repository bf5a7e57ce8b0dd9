#!/usr/bin/env python
"""The cost of a pass boundary (not bench.py's workload): one frame's samples as one ordinary launch, as one
pass and as several, on one device.

  python tools/progressive_probe.py [--scene ultracomplex --width 1920 --height 1080 --spp 64 --splits 1,4,64
                                     --frames 20 --rounds 7 --out profiles/NAME.json]

Variants, each a joined frame on one stream (no RTC_F_OVERLAP: a pass is never pipelined):
  rows        rtc_render_rows_async without an accumulator (the ordinary launch)
  rows_accum  the same with the float accumulator written (what a pass always does)
  passes_N    N equal passes of rtc_render_samples_async covering [0, spp)

After a warm-up of every variant, `--rounds` rounds run the variants one after the other (alternated, so that drift and
other tenants of the machine hit all alike); in a round a variant renders `--frames` frames back to back and is timed by
the host clock around them, ending in a device synchronise.  Printed (one JSON line, also written to --out): per variant
the median, minimum and maximum ms per frame over the rounds, and for N > 1 the overhead per extra pass boundary in
microseconds, (passes_N - passes_1) / (N - 1) from the medians.  Every variant's Color frame must equal the ordinary
launch's byte for byte, or the probe fails."""
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
    ap.add_argument("--splits", default="1,4,64")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    splits = [int(s) for s in a.splits.split(",")]
    if any(n <= 0 or a.spp % n for n in splits):
        raise SystemExit("--splits: pass counts that divide --spp")

    import torch
    from conftest import load_tris, scene_spheres

    import raytracingc_amd as rt

    tris, tonly = load_tris(a.scene)
    sph = scene_spheres(a.scene)
    scene, cam = rt.default_scene(), rt.camera_basis()
    cfg = rt.RenderConfig(a.width, a.height, a.spp, 10, bool(tonly))
    ds = rt.DeviceScene(tris, sph)
    col = torch.zeros((a.height, a.width, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((a.height, a.width, 3), dtype=torch.float32, device="cuda")
    rng = torch.zeros((a.height, a.width), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def rows(accum):
        ds.render_rows_async(scene, cam, cfg, col.data_ptr(), acc.data_ptr() if accum else None, None, st)

    def passes(n):
        for k in range(n):
            ds.render_samples_async(scene, cam, cfg, k * (a.spp // n), a.spp // n, col.data_ptr(), acc.data_ptr(),
                                    rng.data_ptr(), None, st)

    variants = {"rows": lambda: rows(False), "rows_accum": lambda: rows(True)}
    variants.update({f"passes_{n}": (lambda n=n: passes(n)) for n in splits})
    frames, ms = {}, {k: [] for k in variants}
    for name, fn in variants.items():  # warm-up, and every variant's frame
        col.zero_()
        fn()
        fn()
        torch.cuda.synchronize()
        frames[name] = col.cpu()
        if not torch.equal(frames[name], frames["rows"]):
            raise SystemExit(f"{name}: the frame differs from the ordinary launch's")
    for _ in range(a.rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.frames):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    out = {"scene": a.scene, "width": a.width, "height": a.height, "spp": a.spp, "frames": a.frames, "rounds": a.rounds,
           "lib": os.environ.get("RTC_LIB_PATH") or "tree", "checksum": int(frames["rows"].sum(dtype=torch.int64)),
           "ms_per_frame": {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                            for k, v in ms.items()}}
    if "passes_1" in ms:
        one = statistics.median(ms["passes_1"])
        out["us_per_extra_pass"] = {f"passes_{n}": round((statistics.median(ms[f"passes_{n}"]) - one) * 1e3 / (n - 1), 3)
                                    for n in splits if n > 1}
        out["passes_1_minus_rows_accum_us"] = round((one - statistics.median(ms["rows_accum"])) * 1e3, 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ds.close()


if __name__ == "__main__":
    main()
