"""The kernels against calcColor values the reference itself computed (tests/golden/kat_ref_<family>.npz and the model
fixtures kat_calc_<scene>.npz; tests/reference_calc.py states the inputs), with no oracle in between: only committed
fixtures are read.

  path query    rtc_trace_paths at spp 1 is calcColor on a given ray and seed with the RNG state out, with the
                cluster cull and with RTC_F_NO_CLUSTER_CULL;
  render route  the family's frame at one sample per pixel on the default route (rtc_render_rows_async), one whole-frame
                pass of rtc_render_samples_async for the RNG states, and for the families with calcDebugColor values the same
                two under RTC_F_DEBUG_BOUNCES: the render kernels' own primary rays and seeds, read at the fixture's pixels.

The expected radiance is np.float32(0) + colour: main.c:99 with the weight (float)(1. / 1) from a +0 accumulator, whose two
float operations the kernels perform (colour * 1 keeps every bit, +0 + colour turns -0 into +0).  Bit patterns, no
tolerance; where the reference has a NaN any NaN is accepted (the project's standing exception); seeds exactly."""
from __future__ import annotations

import numpy as np
import pytest

import raytracingc_amd as rt
import reference_calc as rc
from conftest import GOLDEN, load_tris, scene_spheres

pytestmark = pytest.mark.gpu

SCENE = rt.default_scene()
FLAGS = (0, rt.RTC_F_NO_CLUSTER_CULL)


def _expected(colour):
    with np.errstate(invalid="ignore"):
        return (np.float32(0) + np.ascontiguousarray(colour, np.float32)).astype(np.float32)


def _against(what, radiance, seeds, colour, seed_after, failures):
    """Print the figures, then note a failure: (records whose radiance differs, records whose seed differs)."""
    bad = rc.differing(radiance, _expected(colour)), int((np.asarray(seeds).view(np.uint32) != seed_after).sum())
    print(f"{what}: {len(seed_after)} records; differing radiance, seeds {bad}")
    if bad != (0, 0):
        failures.append(f"{what}: {bad[0]} radiance and {bad[1]} seeds of {len(seed_after)} differ")


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_path_query(family, gpu_available):
    failures = []
    for case in rc.cases(family):
        rays, seeds, fx = rc.checked_inputs(family, case)
        ds = rt.DeviceScene(case.tris, case.spheres)
        try:
            for flags in FLAGS:
                got = ds.trace_paths(rays, seeds, SCENE, 1, case.max_bounce, bool(case.triangles_only), flags)
                _against(f"{family}/{case.name} flags {flags:#x}", got["radiance"], got["seeds"], fx.color, fx.seed_after,
                         failures)
        finally:
            ds.close()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("scene", ["default", "ultracomplex", "complex"])
def test_path_query_model_fixtures(scene, gpu_available):
    """kat_calc_<scene>.npz: the reference's calcColor on the loaded models (camera rays and rays from inside the scene,
    random seeds), grouped by the records' maxBounce.  maxBounce 0: +0 radiance and the seeds as they were."""
    k = np.load(f"{GOLDEN}/kat_calc_{scene}.npz")
    tris, tonly = load_tris(scene)
    assert sorted(set(k["max_bounce"].tolist())) == [0, 1, 2, 3, 10, 25]
    failures = []
    ds = rt.DeviceScene(tris, scene_spheres(scene))
    try:
        for mb in sorted(set(k["max_bounce"].tolist())):
            m = k["max_bounce"] == mb
            rays, seeds, colour, after = k["rays"][m], k["seeds"][m], k["color"][m], k["seed_after"][m]
            assert m.sum() >= 50
            if mb == 0:
                assert not colour.view(np.uint32).any() and np.array_equal(after, seeds)
            for flags in FLAGS:
                got = ds.trace_paths(rays, seeds, SCENE, 1, mb, bool(tonly), flags)
                if mb == 0:
                    assert not got["radiance"].view(np.uint32).any(), "maxBounce 0: the radiance is +0"
                _against(f"kat_calc_{scene} maxBounce {mb} flags {flags:#x}", got["radiance"], got["seeds"], colour, after,
                         failures)
    finally:
        ds.close()
    assert not failures, "\n".join(failures)


def _frame(ds, case, cfg, samples_pass):
    """(accumulator float32 [pixels, 3], RNG states uint32 [pixels] or None) of the case's frame: one
    rtc_render_rows_async launch, or one whole-frame pass of rtc_render_samples_async."""
    import torch

    H, W = case.height, case.width
    col = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.full((H, W, 3), -1, dtype=torch.int32, device="cuda")  # (0xFF bytes: a first pass must not read them)
    rng = torch.full((H, W), -1, dtype=torch.int32, device="cuda") if samples_pass else None
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    if samples_pass:
        ds.render_samples_async(SCENE, case.camera, cfg, 0, 1, col.data_ptr(), acc.data_ptr(), rng.data_ptr(), None, st)
    else:
        ds.render_rows_async(SCENE, case.camera, cfg, col.data_ptr(), acc.data_ptr(), None, st)
    torch.cuda.synchronize()
    a = acc.cpu().numpy().view(np.float32).reshape(-1, 3)
    return a, (rng.cpu().numpy().view(np.uint32).reshape(-1) if samples_pass else None)


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_render_route(family, gpu_available):
    failures = []
    for case in rc.cases(family):
        _, seeds, fx = rc.checked_inputs(family, case)
        px = case.pixels
        ds = rt.DeviceScene(case.tris, case.spheres)
        try:
            modes = [(False, fx.color, fx.seed_after)]
            if family in rc.DEBUG_FAMILIES:
                modes.append((True, fx.debug_color, fx.debug_seed_after))
            for debug, colour, after in modes:
                cfg = rc.config(case, debug_bounces=debug)
                what = f"{family}/{case.name}{' debug' if debug else ''}"
                acc, _ = _frame(ds, case, cfg, False)
                _against(f"{what} frame", acc[px], after, colour, after, failures)  # (a launch gives no RNG states)
                acc, rng = _frame(ds, case, cfg, True)
                _against(f"{what} pass", acc[px], rng[px], colour, after, failures)
        finally:
            ds.close()
    assert not failures, "\n".join(failures)
