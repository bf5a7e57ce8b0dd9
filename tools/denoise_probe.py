#!/usr/bin/env python
"""Device time of the edge-avoiding denoise filter (rtc_denoise_async) on a real frame, beside the traffic
bound of its passes and a sample pass of the same frame.  Not bench.py's workload.

  python tools/denoise_probe.py [--scene ultracomplex] [--size 1920x1080] [--head 64] [--iterations 5]
                                [--launches 7] [--rounds 3] [--reps 8]

The frame: `head` samples of the scene (render_samples_async) and its first-hit buffers (render_first_hit_async), every
pixel's sample count = head = spp.  Measured, each for the full call (normal, depth, albedo, RTC_DN_DEMODULATE, sample
counts, Color bytes out) and for the bare one (no guides, no sample counts, no Color bytes):
  calls    rtc_denoise_async with 1, 2, .. `iterations` iterations.  A call with K iterations is the pack pass, K - 1
           iterations that write the next 16-byte colour image and one that performs the store step, so the first figure is
           the pack pass plus the step-1 iteration, and the difference between K and K - 1 iterations is what the iteration
           with step 1 << (K - 1) adds (its own time, up to the difference between the two kinds of store).
  copy     the yardstick: a device-to-device copy (a torch copy of a byte tensor) that reads 32 bytes and writes 16 per
           pixel -- an iteration's minimum traffic, 32 B read plus 16 B written per pixel -- and, for the pack pass, one
           that moves the bytes the pack pass reads and writes.
  pass     for context: render_samples_async of `head` further samples of the same frame.
The bound printed beside them: 48 bytes per pixel at 6.3 TB/s (the achievable HBM rate of a float4 copy on an MI355X).
Device figures: `reps` enqueues between two HIP events (torch.cuda.Event), divided by reps; the measurements alternate
launch by launch, `--launches` times per round after one warm-up each; a round's figure is the median of its launches and
the rounds' medians are printed with their spread (max - min over the rounds): a difference inside the spread is none.
One JSON line per measurement, then a markdown table."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_BYTES_PER_MS = 6.3e9  # 6.3 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="ultracomplex")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--head", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--max-bounce", type=int, default=10)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8)
    a = ap.parse_args()
    if a.launches < 5 or a.rounds < 3 or a.reps < 1 or not 1 <= a.iterations <= 6 or a.head < 1:
        raise SystemExit("at least 5 launches per round, 3 rounds, 1 .. 6 iterations")

    import torch

    import raytracingc_amd as rt
    from conftest import load_tris

    if rt.device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    W, H = (int(v) for v in a.size.split("x"))
    n = W * H
    cam, scene = rt.camera_basis(), rt.default_scene()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    cfg = rt.RenderConfig(W, H, 2 * a.head, a.max_bounce, True)

    def timed(launches, extra):
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
                    for _ in range(a.reps):
                        fn()
                    e1.record(st)
                    evs[k].append((e0, e1))
                    torch.cuda.synchronize()
            for k, pairs in evs.items():
                medians[k].append(statistics.median(e0.elapsed_time(e1) / a.reps for e0, e1 in pairs))
        ms = {k: statistics.median(m) for k, m in medians.items()}
        spread = {k: max(m) - min(m) for k, m in medians.items()}
        for k, m in medians.items():
            print(json.dumps({"what": "denoise", **extra, "measurement": list(k), "reps": a.reps,
                              "launches_per_round": a.launches, "round_medians_ms": [round(v, 5) for v in m],
                              "median_ms": round(ms[k], 5), "spread_ms": round(spread[k], 5)}), flush=True)
        return ms, spread

    tris, _ = load_tris(a.scene)
    ds = rt.DeviceScene(tris, None)
    about = {"scene": a.scene, "triangles": len(tris), "size": a.size, "head": a.head}
    col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    rng = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    guides = {"depth": torch.zeros((H, W), dtype=torch.float32, device="cuda"),
              "normal": torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"),
              "albedo": torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")}
    ds.render_samples_async(scene, cam, cfg, 0, a.head, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None, sp)
    ds.render_first_hit_async(cam, cfg, 0, guides["depth"].data_ptr(), guides["normal"].data_ptr(),
                              guides["albedo"].data_ptr(), stream=sp)
    torch.cuda.synchronize()
    frame = acc * 2  # (the accumulator of `head` of 2 * head samples, as a frame of `head` samples)
    samples = torch.full((H, W), a.head, dtype=torch.int32, device="cuda")
    out = torch.empty_like(frame)
    colors = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    nbytes = rt.denoise_scratch_bytes(n, a.iterations)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    launches = {}
    for k in range(1, a.iterations + 1):
        full = rt.denoise_desc(W, H, k, 5, 1.0, 0.05, 0.01, True, a.head)
        bare = rt.denoise_desc(W, H, k, 5, 1.0, 0.05, 0.01, False, 0)
        launches[("full", k)] = lambda d=full: rt.denoise_async(
            frame.data_ptr(), samples.data_ptr(), d, out.data_ptr(), colors.data_ptr(), scratch.data_ptr(), nbytes,
            guides["normal"].data_ptr(), guides["depth"].data_ptr(), guides["albedo"].data_ptr(), sp)
        launches[("bare", k)] = lambda d=bare: rt.denoise_async(frame.data_ptr(), None, d, out.data_ptr(), None,
                                                                scratch.data_ptr(), nbytes, stream=sp)
    pack_bytes = {"full": (12 + 4 + 12 + 4 + 12, 32), "bare": (12, 16)}  # (read, written) per pixel
    src = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    dst = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    # a copy moves as many bytes out as in: 24 B per pixel each way is the iteration's 48 B of traffic
    launches[("copy", "iteration")] = lambda: dst[:24 * n].copy_(src[:24 * n])
    for kind, (rd, wr) in pack_bytes.items():
        half = (rd + wr) // 2
        launches[("copy", "pack " + kind)] = lambda half=half: dst[:half * n].copy_(src[:half * n])
    launches[("pass", a.head)] = lambda: ds.render_samples_async(scene, cam, cfg, a.head, a.head, col.data_ptr(),
                                                                 acc.data_ptr(), rng.data_ptr(), None, sp)
    ms, spread = timed(launches, about)
    ds.close()

    bound = 48 * n / HBM_BYTES_PER_MS
    print(f"\n{a.scene}, {a.size}, a frame of {a.head} samples; ms per call (spread over the rounds)\n")
    print(f"an iteration's minimum traffic, 48 B per pixel: {48 * n / 1e6:.1f} MB, {bound:.4f} ms at 6.3 TB/s; the copy of "
          f"as many bytes: {ms[('copy', 'iteration')]:.4f} ms\n")
    print("| call | full: ms | full: added by the last step | bare: ms | bare: added by the last step |")
    print("|---|---|---|---|---|")
    for k in range(1, a.iterations + 1):
        cells = []
        for kind in ("full", "bare"):
            t = ms[(kind, k)]
            cells.append(f"{t:.4f} ({spread[(kind, k)]:.4f})")
            cells.append("pack + step 1" if k == 1 else f"step {1 << (k - 1)}: {t - ms[(kind, k - 1)]:.4f}")
        print(f"| {k} iteration{'s' if k > 1 else ''} | " + " | ".join(cells) + " |")
    print()
    for kind, (rd, wr) in pack_bytes.items():
        print(f"the pack pass, {kind}: {rd} B read and {wr} B written per pixel, {(rd + wr) * n / HBM_BYTES_PER_MS:.4f} ms at "
              f"6.3 TB/s; the copy of as many bytes: {ms[('copy', 'pack ' + kind)]:.4f} ms")
    print(f"a pass of {a.head} samples over the same frame: {ms[('pass', a.head)]:.4f} ms "
          f"({spread[('pass', a.head)]:.4f})\n")


if __name__ == "__main__":
    main()
