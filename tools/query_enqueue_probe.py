#!/usr/bin/env python
"""Host cost of the three ray queries' entries: wall-clock microseconds per call of each *_async entry
(65 rays on the default scene, batches of 200 calls, the stream synchronised between batches and outside the timed
region) and of each host entry (batches of 50 calls, which synchronise themselves).  Not bench.py's workload.

  python tools/query_enqueue_probe.py [label]

Per entry: the batches' per-call figures, their median and their spread (max - min).  One JSON line per entry; run it
for two trees alternately, several times each: the spread between one tree's runs is the yardstick for a difference."""
import json
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
label = sys.argv[1] if len(sys.argv) > 1 else "tree"
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import raytracingc_amd as rt  # noqa: E402
from conftest import load_tris, scene_spheres  # noqa: E402
from primary_rays import launch_rays  # noqa: E402

N = 65
ds = rt.DeviceScene(load_tris("default")[0], scene_spheres("default"))
scene = rt.default_scene()
host = np.ascontiguousarray(launch_rays(rt.camera_basis(), rt.RenderConfig(64, 40, 0, 0, False))[:N])
rays = torch.from_numpy(host.view(np.float32).reshape(-1, 6).copy()).cuda()
seeds_h = np.arange(N, dtype=np.uint32)
seeds = torch.from_numpy(seeds_h.view(np.int32).copy()).cuda()
prim = torch.zeros(N, dtype=torch.int32, device="cuda")
depth = torch.zeros(N, dtype=torch.float32, device="cuda")
nrm = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
alb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
rad = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
sout = torch.zeros(N, dtype=torch.int32, device="cuda")
occ = torch.zeros(N, dtype=torch.uint8, device="cuda")
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
st = torch.cuda.current_stream().cuda_stream

ASYNC = {
    "rtc_trace_rays_async": lambda: ds.trace_rays_async(rays.data_ptr(), N, False, 0, prim.data_ptr(), depth.data_ptr(),
                                                        nrm.data_ptr(), alb.data_ptr(), stream=st),
    "rtc_trace_paths_async": lambda: ds.trace_paths_async(scene, rays.data_ptr(), seeds.data_ptr(), N, 1, 2, rad.data_ptr(),
                                                          False, 0, 0, 1, sout.data_ptr(), 0, stream=st),
    "rtc_occluded_async": lambda: ds.occluded_async(rays.data_ptr(), N, 0, False, 0, occ.data_ptr(), cnt.data_ptr(),
                                                    stream=st),
}
HOST = {
    "rtc_trace_rays": lambda: ds.trace_rays(host),
    "rtc_trace_paths": lambda: ds.trace_paths(host, seeds_h, scene, 1, 2),
    "rtc_occluded": lambda: ds.occluded(host, None, False, 0, count=True),
}


def measure(name, call, per_batch, batches):
    for _ in range(per_batch):  # warm-up
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(per_batch):
            call()
        us.append((time.perf_counter() - t0) / per_batch * 1e6)
        torch.cuda.synchronize()
    print(json.dumps({"tree": label, "entry": name, "calls_per_batch": per_batch, "us_per_call": [round(v, 2) for v in us],
                      "median_us": round(statistics.median(us), 2), "spread_us": round(max(us) - min(us), 2)}), flush=True)


for k, f in ASYNC.items():
    measure(k, f, 200, 10)
for k, f in HOST.items():
    measure(k, f, 50, 6)
