#!/usr/bin/env python
"""Device time of a pass over a list of pixels (rtc_render_pixels_async) beside the whole pass it replaces
for an adaptive frame's tail.  Not bench.py's workload.

  python tools/render_pixels_probe.py [--scenes ultracomplex,fsuzane] [--size 1920x1080] [--spp 1024] [--head 64]
                                      [--max-bounce 10] [--launches 7] [--rounds 3]

Per scene, one progressive frame of --spp samples: a whole pass [0, head) (rtc_render_samples_async), then
  whole        one more whole pass of `head` samples, [head, 2 head): the yardstick
  lane / wave  pixel passes [head, 2 head) and [head, spp) -- 64 and 960 samples by default -- over the 100 %, 10 %, 1 %
               and 0.1 % of the pixels whose accumulator after the first pass differs most from their right neighbour's
               (sum of the three absolute differences; 100 %: every pixel), with the lane-per-pixel kernel and the
               wave-per-pixel kernel (RTC_F_WAVE_PER_RAY), the list in raster order and in a fixed random permutation.
Before every timed launch the frame's accumulator and states are put back to what the first pass left (device copies,
outside the timed interval), so every launch of a measurement does the same work.  Each launch lies between two HIP
events (torch.cuda.Event); the measurements alternate launch by launch, `--launches` times per round after one warm-up
each; a round's figure is the median of its launches and the rounds' medians are printed with their spread (max - min over
the rounds): a difference inside the spread is none.  Before anything is timed, a pixel pass over every pixel must leave
the whole pass's accumulator, states and Color, word for word, with both kernels.
One JSON line per measurement, then per scene a table (markdown) and, per kernel and order, the break-even share: where, by
linear interpolation in the logarithm of the share between the two measured shares around it, a pixel pass of `head`
samples costs what the whole pass of `head` samples costs."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SHARES = (1.0, 0.1, 0.01, 0.001)


def break_even(shares, times, yardstick):
    """The share at which the pixel pass costs `yardstick`: None when every share is cheaper, 0 when none is."""
    pts = sorted(zip(shares, times))
    if all(t <= yardstick for _, t in pts):
        return None
    if all(t > yardstick for _, t in pts):
        return 0.0
    for (s0, t0), (s1, t1) in zip(pts, pts[1:]):
        if t0 <= yardstick < t1:
            f = (yardstick - t0) / (t1 - t0)
            return math.exp(math.log(s0) + f * (math.log(s1) - math.log(s0)))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="ultracomplex,fsuzane")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--head", type=int, default=64)
    ap.add_argument("--max-bounce", type=int, default=10)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.launches < 5 or a.rounds < 3 or not 0 < 2 * a.head <= a.spp:
        raise SystemExit("at least 5 launches per round, 3 rounds, and 2 * head <= spp")

    import numpy as np
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
    tail = a.spp - a.head
    perm_rng = np.random.default_rng(2024)

    for name in a.scenes.split(","):
        tris, _ = load_tris(name)
        ds = rt.DeviceScene(tris, None)
        col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        rng = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        ds.render_samples_async(scene, cam, cfg, 0, a.head, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None, sp)
        torch.cuda.synchronize()
        acc0, rng0, col0 = acc.clone(), rng.clone(), col.clone()

        def restore():
            acc.copy_(acc0)
            rng.copy_(rng0)

        # the lists: the pixels whose sum differs most from their right neighbour's
        diff = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        diff[:, :-1] = (acc0[:, :-1] - acc0[:, 1:]).abs().sum(-1)
        order = torch.argsort(diff.reshape(-1), descending=True, stable=True).cpu().numpy()
        lists = {}
        for share in SHARES:
            k = n if share == 1.0 else max(1, int(round(n * share)))
            raster = np.sort(order[:k]).astype(np.uint32)
            lists[share] = {"raster": torch.from_numpy(raster.view(np.int32).copy()).cuda(),
                            "permuted": torch.from_numpy(perm_rng.permutation(raster).view(np.int32).copy()).cuda()}

        def whole():
            ds.render_samples_async(scene, cam, cfg, a.head, a.head, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None, sp)

        def pixels(lst, count, flags):
            return lambda: ds.render_pixels_async(scene, cam, cfg, a.head, count, lst.data_ptr(), lst.numel(), acc.data_ptr(),
                                                  rng.data_ptr(), col.data_ptr(), None, flags, sp)

        # a pixel pass over every pixel is the whole pass, before anything is timed
        restore()
        whole()
        torch.cuda.synchronize()
        want = acc.clone(), rng.clone(), col.clone()
        for kernel, flags in (("lane", 0), ("wave", rt.RTC_F_WAVE_PER_RAY)):
            restore()
            col.copy_(col0)
            pixels(lists[1.0]["permuted"], a.head, flags)()
            torch.cuda.synchronize()
            ok = all(bool((g.view(torch.uint8) == w.view(torch.uint8)).all().item()) for g, w in zip((acc, rng, col), want))
            print(json.dumps({"what": "check", "scene": name, "kernel": kernel, "pixels": n, "samples": a.head,
                              "equals_whole_pass": ok}), flush=True)
            if not ok:
                raise SystemExit("the pixel pass and the whole pass disagree")

        launches = {("whole", 1.0, "raster", a.head): whole}
        for count in (a.head, tail):
            for share in SHARES:
                for kernel, flags in (("lane", 0), ("wave", rt.RTC_F_WAVE_PER_RAY)):
                    for how in ("raster", "permuted"):
                        launches[(kernel, share, how, count)] = pixels(lists[share][how], count, flags)
        for fn in launches.values():  # the warm-up of every one
            restore()
            fn()
        torch.cuda.synchronize()
        medians = {k: [] for k in launches}
        for r in range(a.rounds):
            print(json.dumps({"what": "round", "scene": name, "round": r}), flush=True)
            evs = {k: [] for k in launches}
            for _ in range(a.launches):
                for k, fn in launches.items():
                    restore()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    evs[k].append((e0, e1))
                    torch.cuda.synchronize()  # (bounds the queue: a launch here is milliseconds)
            for k, pairs in evs.items():
                medians[k].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs))
        ms = {k: statistics.median(m) for k, m in medians.items()}
        for (kernel, share, how, count), m in medians.items():
            print(json.dumps({"what": "launch", "scene": name, "triangles": len(tris), "size": a.size, "spp": a.spp,
                              "max_bounce": a.max_bounce, "kernel": kernel, "share": share,
                              "pixels": lists[share][how].numel() if kernel != "whole" else n, "order": how, "samples": count,
                              "launches_per_round": a.launches, "round_medians_ms": [round(v, 4) for v in m],
                              "median_ms": round(ms[(kernel, share, how, count)], 4),
                              "spread_ms": round(max(m) - min(m), 4)}), flush=True)
        yard = ms[("whole", 1.0, "raster", a.head)]
        print(f"\n{name}, {a.size}, spp {a.spp}, maxBounce {a.max_bounce}: whole pass of {a.head} samples {yard:.3f} ms\n")
        print(f"| samples | share | pixels | lane raster | lane permuted | wave raster | wave permuted |")
        print(f"|---|---|---|---|---|---|---|")
        for count in (a.head, tail):
            for share in SHARES:
                cells = [f"{ms[(k, share, how, count)]:.3f}" for k in ("lane", "wave") for how in ("raster", "permuted")]
                print(f"| {count} | {share * 100:g} % | {lists[share]['raster'].numel()} | " + " | ".join(cells) + " |")
        for kernel in ("lane", "wave"):
            for how in ("raster", "permuted"):
                be = break_even(SHARES, [ms[(kernel, s, how, a.head)] for s in SHARES], yard)
                text = "never (cheaper at every share)" if be is None else "none (dearer at every share)" if be == 0 else \
                    f"{be * 100:.2f} %"
                print(json.dumps({"what": "break_even", "scene": name, "kernel": kernel, "order": how, "samples": a.head,
                                  "whole_pass_ms": round(yard, 4), "share": text}), flush=True)
        ds.close()


if __name__ == "__main__":
    main()
