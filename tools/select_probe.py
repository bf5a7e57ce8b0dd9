#!/usr/bin/env python
"""Device time of the adaptive frame's select (rtc_select_pixels_async), of the host round trip it replaces
and of the sentinel padding it hands to the pixel pass.  Not bench.py's workload.

  python tools/select_probe.py [--scenes ultracomplex,fsuzane] [--size 1920x1080] [--spp 1024] [--head 64]
                               [--max-bounce 10] [--launches 7] [--rounds 3] [--reps 8] [--only select,host,padding]

Per scene, one progressive frame of --spp samples after two whole passes of `head` samples (the snapshot is the accumulator
after the first).
  select   rtc_select_pixels_async (list out at capacity = the input's length, count, samples stamped) over every pixel and
           over lists of 10 %, 1 % and 0.1 % of the frame (the pixels with the largest d * d / (l + floor), in raster order;
           the threshold is the list's median of that ratio, so about half of every input goes on); `judge` is the same call
           with neither list nor count, which enqueues the judge kernel alone; `copy` is the yardstick: a device-to-device
           hipMemcpyAsync (a torch copy of a byte tensor) of the bytes the select reads, 24 per entry without a list and 28
           with one; `snapshot` is the device-to-device copy of the whole accumulator the device loop makes per pass.
  host     the step the device loop replaces: DeviceScene.render_adaptive's wall time for one further pass over ONE pixel
           with ONE sample behind a trivial `select` -- the callback, the upload of the list, the synchronisation and the
           copies of accumulator and Color to the host (this mode uses nothing the parent commit's library lacks: run it
           with RTC_LIB_PATH naming that library).
  padding  rtc_render_pixels_async over a list of nothing but 0xFFFFFFFF, as long as 0.1 %, 1 % and 10 % of the frame, with
           both kernels: what a capacity that is never filled costs the next pass.
Device figures: `reps` enqueues between two HIP events (torch.cuda.Event), divided by reps; the measurements alternate
launch by launch, `--launches` times per round after one warm-up each; a round's figure is the median of its launches and
the rounds' medians are printed with their spread (max - min over the rounds): a difference inside the spread is none.
One JSON line per measurement, then per scene markdown tables."""
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

SHARES = (1.0, 0.1, 0.01, 0.001)
FLOOR = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="ultracomplex,fsuzane")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--head", type=int, default=64)
    ap.add_argument("--max-bounce", type=int, default=10)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--only", default="select,host,padding")
    a = ap.parse_args()
    modes = set(a.only.split(","))
    if a.launches < 5 or a.rounds < 3 or a.reps < 1 or not 0 < 2 * a.head < a.spp or not modes <= {"select", "host", "padding"}:
        raise SystemExit("at least 5 launches per round, 3 rounds, 2 * head < spp, --only of select, host, padding")

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
    cfg = rt.RenderConfig(W, H, a.spp, a.max_bounce, True)

    def timed(launches, what, extra):
        """`launches`: name -> function that enqueues the work once.  Prints one JSON line each; returns name -> median ms."""
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
        for k, m in medians.items():
            print(json.dumps({"what": what, **extra, "measurement": list(k) if isinstance(k, tuple) else k,
                              "reps": a.reps, "launches_per_round": a.launches,
                              "round_medians_ms": [round(v, 5) for v in m], "median_ms": round(ms[k], 5),
                              "spread_ms": round(max(m) - min(m), 5)}), flush=True)
        return ms

    for name in a.scenes.split(","):
        tris, _ = load_tris(name)
        ds = rt.DeviceScene(tris, None)
        about = {"scene": name, "triangles": len(tris), "size": a.size, "spp": a.spp, "head": a.head}

        if "host" in modes:
            walls = []
            for _ in range(a.rounds * a.launches):
                gen = ds.render_adaptive(scene, cam, cfg, [a.head, 1], lambda done, col, acc, smp: [0])
                next(gen)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                next(gen)  # select, upload of the list, a pass of one sample over one pixel, synchronise, two copies to the host
                walls.append((time.perf_counter() - t0) * 1e3)
                gen.close()
            walls.sort()
            print(json.dumps({"what": "host_step", **about,
                              "library": "RTC_LIB_PATH" if os.environ.get("RTC_LIB_PATH") else "the tree's", "steps": len(walls),
                              "median_ms": round(statistics.median(walls), 3), "min_ms": round(walls[0], 3),
                              "max_ms": round(walls[-1], 3)}), flush=True)
            print(f"\n{name}, {a.size}: render_adaptive's step between two passes (one pixel, one sample): median "
                  f"{statistics.median(walls):.3f} ms, min {walls[0]:.3f}, max {walls[-1]:.3f} over {len(walls)} steps\n")

        if "padding" in modes:
            acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            rng = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            launches = {}
            for share in SHARES[1:]:
                pad = torch.full((max(1, int(round(n * share))),), -1, dtype=torch.int32, device="cuda")
                for kernel, flags in (("lane", 0), ("wave", rt.RTC_F_WAVE_PER_RAY)):
                    launches[(kernel, share, pad.numel())] = (
                        lambda pad=pad, flags=flags: ds.render_pixels_async(scene, cam, cfg, a.head, a.head, pad.data_ptr(),
                                                                            pad.numel(), acc.data_ptr(), rng.data_ptr(), 0,
                                                                            None, flags, sp))
            ms = timed(launches, "padding", about)
            assert not bool(acc.any().item()) and not bool(rng.any().item()), "a sentinel was rendered"
            print(f"\n{name}, {a.size}: a pixel pass over nothing but sentinels, ms per launch\n")
            print("| capacity | entries | lane | wave |\n|---|---|---|---|")
            for share in SHARES[1:]:
                k = max(1, int(round(n * share)))
                print(f"| {share * 100:g} % | {k} | {ms[('lane', share, k)]:.4f} | {ms[('wave', share, k)]:.4f} |")
            print()

        if "select" in modes:
            col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            rng = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            ds.render_samples_async(scene, cam, cfg, 0, a.head, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None, sp)
            prev = acc.clone()
            ds.render_samples_async(scene, cam, cfg, a.head, a.head, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None, sp)
            torch.cuda.synchronize()
            d = rt.select_desc(a.spp, a.head, 2 * a.head, 1.0, FLOOR)
            e = (acc * d.wAccum - prev * d.wPrev).abs().sum(-1)
            ratio = torch.nan_to_num((e * e / (acc.sum(-1) * d.wLevel + d.floor)).reshape(-1), nan=0.0)
            order = torch.argsort(ratio, descending=True, stable=True)
            samples = torch.zeros(n, dtype=torch.int32, device="cuda")
            count = torch.zeros(1, dtype=torch.int64, device="cuda")
            nbytes = rt.select_scratch_bytes(n)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            snap = torch.empty_like(acc)
            launches, sizes = {("snapshot", 1.0): lambda: snap.copy_(acc)}, {}
            for share in SHARES:
                k = n if share == 1.0 else max(1, int(round(n * share)))
                lst = None if share == 1.0 else torch.sort(order[:k]).values.to(torch.int32).contiguous()
                mid = float(torch.median(ratio if lst is None else ratio[lst.long()]).item())
                sel = rt.select_desc(a.spp, a.head, 2 * a.head, mid, FLOOR)
                out = torch.empty(k, dtype=torch.int32, device="cuda")
                src = torch.empty(k * (24 if lst is None else 28), dtype=torch.uint8, device="cuda")
                dst = torch.empty_like(src)
                inp, n_in = (None, 0) if lst is None else (lst.data_ptr(), k)

                def select(sel=sel, inp=inp, n_in=n_in, out=out, k=k):
                    rt.select_pixels_async(acc.data_ptr(), prev.data_ptr(), n, inp, n_in, sel, out.data_ptr(), k,
                                           count.data_ptr(), samples.data_ptr(), scratch.data_ptr(), nbytes, sp)

                def judge(sel=sel, inp=inp, n_in=n_in):
                    rt.select_pixels_async(acc.data_ptr(), prev.data_ptr(), n, inp, n_in, sel, None, 0, None,
                                           samples.data_ptr(), scratch.data_ptr(), nbytes, sp)

                select()
                torch.cuda.synchronize()
                sizes[share] = (k, int(count.item()), src.numel())
                launches[("select", share)] = select
                launches[("judge", share)] = judge
                launches[("copy", share)] = lambda src=src, dst=dst: dst.copy_(src)
            ms = timed(launches, "select", about)
            print(f"\n{name}, {a.size}, after two whole passes of {a.head}: ms per call; GB/s = the bytes read over the time\n")
            print("| input | entries | selected | bytes read | select | judge alone | copy of those bytes | judge GB/s | copy GB/s |")
            print("|---|---|---|---|---|---|---|---|---|")
            for share in SHARES:
                k, chosen, nb = sizes[share]
                print(f"| {'every pixel' if share == 1.0 else f'list, {share * 100:g} %'} | {k} | {chosen} | {nb} | "
                      f"{ms[('select', share)]:.4f} | {ms[('judge', share)]:.4f} | {ms[('copy', share)]:.4f} | "
                      f"{nb / ms[('judge', share)] / 1e6:.0f} | {nb / ms[('copy', share)] / 1e6:.0f} |")
            print(f"\nthe device loop's step: snapshot {ms[('snapshot', 1.0)]:.4f} ms + select over every pixel "
                  f"{ms[('select', 1.0)]:.4f} ms = {ms[('snapshot', 1.0)] + ms[('select', 1.0)]:.4f} ms\n")
        ds.close()


if __name__ == "__main__":
    main()
