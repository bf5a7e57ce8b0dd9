#!/usr/bin/env python
"""Device time of the path query (rtc_trace_paths_async) on a frame's worth of rays, with and without the
cluster cull, coherent and incoherent, beside the render launches that give the same radiance for camera rays.  Not
bench.py's workload.

  python tools/trace_paths_probe.py [--scene ultracomplex] [--size 1920x1080] [--spp 64] [--max-bounce 10]
                                    [--launches 30] [--rounds 3]

The rays are the primary rays of the golden camera's frame (tests/primary_rays.launch_rays: 2,073,600 at 1080p) with the
pixels' seeds x + y * width, so the query's radiance is the frame's accumulator.  Eight launches on one stream, each between
two HIP events (torch.cuda.Event), after a warm-up of every one:
  a query_cull          the rays in raster order, the cluster hierarchy
  b query_brute         ... with RTC_F_NO_CLUSTER_CULL (every record, reference order)
  c rows_nocoop         rtc_render_rows_async with RTC_F_NO_COOP: one lane per pixel, today's route to the same numbers
  d rows_default        the default split launch
  e query_cull_perm     (a) with the rays and seeds in a fixed random permutation
  f query_brute_perm    (b) likewise
  g box_query_cull      (a) on the default box with its sphere (every path bounces until the roulette or maxBounce ends it)
  h box_rows_nocoop     (c) there: its bounce rays test every triangle, the query's use the hierarchy
They alternate launch by launch, `--launches` times per round; a round's figure is the median of its launches, and the
rounds' medians with their spread (max - min over the rounds) are printed: a difference inside the spread is none.  Before
anything is timed the query's radiance (a, b, and e, f permuted back) must equal the accumulator of (c), and (g) that of
(h), as uint32 words, NaN for NaN.  One JSON line per measurement.

  python tools/trace_paths_probe.py --wave [--launches 30] [--rounds 3]

RTC_F_WAVE_PER_RAY against the lane kernel (flags 0, the baseline), under the same protocol, on four legs:
  i   wave_hits     4,096 of the frame's geometry-hitting rays (evenly spaced among them), spp 1,024: few rays, many samples
  ii  wave_sky      4,096 of its sky rays, spp 1,024
  iii wave_frame    the whole frame's rays at --spp (64): (a) above
  iv  wave_box      4,096 evenly spaced rays of the default box's frame, spp 1,024
Each leg times `lane` and `wave` alternately, after `--warmup` launches of both.  Before anything is timed the two kernels' radiance, seeds and segment count
must be equal word for word (NaN for NaN) on every leg."""
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
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--max-bounce", type=int, default=10)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--wave", action="store_true", help="RTC_F_WAVE_PER_RAY against the lane kernel (legs i-iv)")
    ap.add_argument("--few", type=int, default=4096, help="--wave: the rays of legs i, ii and iv")
    ap.add_argument("--many-spp", type=int, default=1024, help="--wave: the samples of legs i, ii and iv")
    a = ap.parse_args()
    if a.launches < 20:
        raise SystemExit("at least 20 launches per round")

    import numpy as np
    import torch

    import raytracingc_amd as rt
    from conftest import load_tris, scene_spheres
    from primary_rays import launch_rays

    if rt.device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    W, H = (int(v) for v in a.size.split("x"))
    cam, scene = rt.camera_basis(), rt.default_scene()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    no_cull = rt.RTC_F_NO_CLUSTER_CULL

    def same(x, y):
        x, y = x.reshape(-1), y.reshape(-1)
        return bool(((x.view(torch.int32) == y.view(torch.int32)) | (torch.isnan(x) & torch.isnan(y))).all().item())

    def setup(tris, spheres, tonly):
        """The device scene, the rays in raster and permuted order with their seeds, and the launches."""
        ds = rt.DeviceScene(tris, spheres)
        host = launch_rays(cam, rt.RenderConfig(W, H, 0, 0, tonly)).view(np.float32).reshape(-1, 6)
        n = len(host)
        seeds = np.arange(n, dtype=np.uint32).view(np.int32)
        perm = np.random.default_rng(2024).permutation(n)
        dev = {"rays": torch.from_numpy(host.copy()).cuda(), "seeds": torch.from_numpy(seeds.copy()).cuda(),
               "rays_perm": torch.from_numpy(host[perm].copy()).cuda(), "seeds_perm": torch.from_numpy(seeds[perm].copy()).cuda(),
               "perm": torch.from_numpy(perm).cuda(), "rad": torch.zeros((n, 3), dtype=torch.float32, device="cuda"),
               "col": torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda"),
               "acc": torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")}

        def query(flags, permuted=False):
            r, s = (dev["rays_perm"], dev["seeds_perm"]) if permuted else (dev["rays"], dev["seeds"])
            return lambda: ds.trace_paths_async(scene, r.data_ptr(), s.data_ptr(), n, a.spp, a.max_bounce,
                                                dev["rad"].data_ptr(), tonly, flags, stream=sp)

        def rows(**kw):
            cfg = rt.RenderConfig(W, H, a.spp, a.max_bounce, tonly, **kw)
            return lambda: ds.render_rows_async(scene, cam, cfg, dev["col"].data_ptr(), dev["acc"].data_ptr(), None, sp)

        return ds, n, dev, query, rows

    tris, _ = load_tris(a.scene)
    box_tris, _ = load_tris("default")
    if a.wave:
        return wave_legs(a, rt, np, torch, tris, box_tris, scene_spheres("default"), cam, scene, st, same)
    ds, n, dev, query, rows = setup(tris, None, True)
    bds, bn, bdev, bquery, brows = setup(box_tris, scene_spheres("default"), False)
    launches = {
        "a query_cull": query(0), "b query_brute": query(no_cull), "c rows_nocoop": rows(coop=False), "d rows_default": rows(),
        "e query_cull_perm": query(0, True), "f query_brute_perm": query(no_cull, True),
        "g box_query_cull": bquery(0), "h box_rows_nocoop": brows(coop=False),
    }
    # the routes to the same numbers agree before anything is timed
    launches["c rows_nocoop"]()
    launches["h box_rows_nocoop"]()
    torch.cuda.synchronize()
    for name, d, permuted in (("a query_cull", dev, False), ("b query_brute", dev, False), ("e query_cull_perm", dev, True),
                              ("f query_brute_perm", dev, True), ("g box_query_cull", bdev, False)):
        d["rad"].fill_(-1.0)
        launches[name]()
        torch.cuda.synchronize()
        want = d["acc"].reshape(-1, 3)
        ok = same(d["rad"], want[d["perm"]] if permuted else want)
        print(json.dumps({"what": "check", "launch": name, "equals_rows_nocoop": ok, "rays": len(want)}), flush=True)
        if not ok:
            raise SystemExit("the path query and the render launch disagree")
    for _ in range(a.warmup):
        for fn in launches.values():
            fn()
    torch.cuda.synchronize()
    medians = {k: [] for k in launches}
    for r in range(a.rounds):
        evs = {k: [] for k in launches}
        for _ in range(a.launches):
            for k, fn in launches.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                evs[k].append((e0, e1))
            torch.cuda.synchronize()  # (bounds the queue: a launch here is milliseconds, not microseconds)
        for k, pairs in evs.items():
            medians[k].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs))
        print(json.dumps({"what": "round", "round": r, "medians_ms": {k: round(m[-1], 4) for k, m in medians.items()}}),
              flush=True)
    for k, m in medians.items():
        box = k[0] in "gh"
        rays = bn if box else n
        print(json.dumps({"what": "launch", "scene": "default+sphere" if box else a.scene,
                          "triangles": len(box_tris if box else tris), "size": a.size, "rays": rays, "spp": a.spp,
                          "max_bounce": a.max_bounce, "launch": k, "launches_per_round": a.launches,
                          "round_medians_ms": [round(v, 4) for v in m], "median_ms": round(statistics.median(m), 4),
                          "spread_ms": round(max(m) - min(m), 4),
                          "ns_per_ray_sample": round(statistics.median(m) * 1e6 / (rays * a.spp), 4)}), flush=True)
    ds.close()
    bds.close()


def wave_legs(a, rt, np, torch, tris, box_tris, box_spheres, cam, scene, st, same):
    """--wave: the lane kernel and the wave kernel, alternating, on the four legs of the module's description."""
    from primary_rays import launch_rays

    W, H = (int(v) for v in a.size.split("x"))
    sp = st.cuda_stream
    wave = rt.RTC_F_WAVE_PER_RAY

    def pick(idx, count):
        """`count` of the indices, evenly spaced."""
        if len(idx) < count:
            raise SystemExit(f"only {len(idx)} rays to take {count} from")
        return idx[(np.arange(count) * len(idx)) // count]

    ds, bds = rt.DeviceScene(tris, None), rt.DeviceScene(box_tris, box_spheres)
    host = launch_rays(cam, rt.RenderConfig(W, H, 0, 0, True)).view(np.float32).reshape(-1, 6)
    bhost = launch_rays(cam, rt.RenderConfig(W, H, 0, 0, False)).view(np.float32).reshape(-1, 6)
    prim = ds.trace_rays(torch.from_numpy(host.copy()).cuda(), True, want=("prim",))["prim"]
    everything = np.arange(len(host))
    legs = {}
    for name, d, tonly, rays, idx, spp in (
            ("i wave_hits", ds, True, host, pick(np.flatnonzero(prim >= 0), a.few), a.many_spp),
            ("ii wave_sky", ds, True, host, pick(np.flatnonzero(prim < 0), a.few), a.many_spp),
            ("iii wave_frame", ds, True, host, everything, a.spp),
            ("iv wave_box", bds, False, bhost, pick(everything, a.few), a.many_spp)):
        n = len(idx)
        buf = {"rays": torch.from_numpy(rays[idx].copy()).cuda(),
               "seeds": torch.from_numpy(idx.astype(np.uint32).view(np.int32).copy()).cuda()}
        out = {k: (torch.zeros((n, 3), dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
                   torch.zeros(1, dtype=torch.int64, device="cuda")) for k in ("lane", "wave")}

        def launch(kind, d=d, tonly=tonly, n=n, spp=spp, buf=buf, out=out):
            rad, seeds_out, seg = out[kind]
            return lambda: d.trace_paths_async(scene, buf["rays"].data_ptr(), buf["seeds"].data_ptr(), n, spp, a.max_bounce,
                                               rad.data_ptr(), tonly, wave if kind == "wave" else 0,
                                               seeds_out_ptr=seeds_out.data_ptr(), segments_ptr=seg.data_ptr(), stream=sp)

        legs[name] = {"n": n, "spp": spp, "out": out, "lane": launch("lane"), "wave": launch("wave"),
                      "triangles": len(box_tris if d is bds else tris)}
    # the two kernels agree word for word before anything is timed (this is the warm-up of both as well)
    for name, leg in legs.items():
        for kind in ("lane", "wave"):
            leg["out"][kind][0].fill_(-1.0)
            leg[kind]()
        torch.cuda.synchronize()
        (lr, ls, lg), (wr, wsd, wg) = leg["out"]["lane"], leg["out"]["wave"]
        ok = same(lr, wr) and bool((ls == wsd).all().item()) and int(lg.item()) == int(wg.item())
        print(json.dumps({"what": "check", "leg": name, "rays": leg["n"], "spp": leg["spp"], "wave_equals_lane": ok,
                          "segments": int(lg.item())}), flush=True)
        if not ok:
            raise SystemExit("the lane kernel and the wave kernel disagree")
    for name, leg in legs.items():
        for _ in range(a.warmup):
            for kind in ("lane", "wave"):
                leg[kind]()
        torch.cuda.synchronize()
        medians = {"lane": [], "wave": []}
        for r in range(a.rounds):
            evs = {"lane": [], "wave": []}
            for _ in range(a.launches):
                for kind in ("lane", "wave"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    leg[kind]()
                    e1.record(st)
                    evs[kind].append((e0, e1))
                torch.cuda.synchronize()
            for kind, pairs in evs.items():
                medians[kind].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs))
        spread = max(max(m) - min(m) for m in medians.values())
        lane_ms, wave_ms = (statistics.median(medians[k]) for k in ("lane", "wave"))
        for kind, m in medians.items():
            print(json.dumps({"what": "launch", "leg": name, "kernel": kind, "triangles": leg["triangles"], "size": a.size,
                              "rays": leg["n"], "spp": leg["spp"], "max_bounce": a.max_bounce,
                              "launches_per_round": a.launches, "round_medians_ms": [round(v, 4) for v in m],
                              "median_ms": round(statistics.median(m), 4), "spread_ms": round(max(m) - min(m), 4),
                              "ns_per_ray_sample": round(statistics.median(m) * 1e6 / (leg["n"] * leg["spp"]), 4)}),
                  flush=True)
        gain = lane_ms - wave_ms
        verdict = "wave wins" if gain >= 3 * spread else "wave loses" if -gain >= 3 * spread else "inside the spread"
        print(json.dumps({"what": "leg", "leg": name, "lane_ms": round(lane_ms, 4), "wave_ms": round(wave_ms, 4),
                          "lane_over_wave": round(lane_ms / wave_ms, 3), "larger_spread_ms": round(spread, 4),
                          "verdict": verdict}), flush=True)
    ds.close()
    bds.close()


if __name__ == "__main__":
    main()
