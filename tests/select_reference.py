"""The selection statement and the sequence semantics of rtc_select_pixels_async / rtc_select_pixels_host (include/rtc.h,
DESIGN §3.20) restated in numpy, with no code under test in the loop, the designed value sets both are held to, and the
CPU reference of a whole adaptive frame (DeviceScene.render_adaptive_device) built on tests/pixel_pass_reference.py.

The statement, float32 operation by operation (numpy rounds every float32 operation to float32 and keeps subnormals):
    e_c = |A_c * wAccum - P_c * wPrev|;  d = (e_x + e_y) + e_z;  l = ((A_x + A_y) + A_z) * wLevel
    selected = d * d > threshold * (l + floor)            (strict; false for any NaN)
The sequence: the input is `pixels`, or 0 .. pixel count - 1; an entry >= the pixel count is invalid (skipped: not judged,
not stamped); the selected valid entries in input order, cut at `capacity`, then 0xFFFFFFFF up to `capacity`; the count is
the number selected before the cut; every valid entry's sample count becomes desc.samplesDone."""
from __future__ import annotations

import types

import numpy as np

F = np.float32
SENTINEL = 0xFFFFFFFF
INF, NAN = F(np.inf), F(np.nan)


def desc(w_accum, w_prev, w_level, floor, threshold, samples_done=0):
    """The six fields of an RtcSelectDesc, the five floats rounded to float32 once."""
    return types.SimpleNamespace(wAccum=F(w_accum), wPrev=F(w_prev), wLevel=F(w_level), floor=F(floor),
                                 threshold=F(threshold), samplesDone=int(samples_done))


def frame_desc(spp, before, done, threshold, floor):
    """The desc that compares the mean of samples [before, done) with the mean of samples [0, before): the weights in
    double, rounded once."""
    w = np.float64(spp) / np.float64(done - before)
    return desc(w, w + np.float64(spp) / np.float64(before), np.float64(spp) / np.float64(done), floor, threshold, done)


def selected(A, P, s):
    """bool [n] for accumulators A and snapshots P, float32 [n, 3]."""
    A, P = np.asarray(A, F).reshape(-1, 3), np.asarray(P, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = np.abs(A * s.wAccum - P * s.wPrev)
        d = (e[:, 0] + e[:, 1]) + e[:, 2]
        lvl = ((A[:, 0] + A[:, 1]) + A[:, 2]) * s.wLevel
        assert e.dtype == d.dtype == lvl.dtype == F
        return d * d > s.threshold * (lvl + s.floor)


def select(accum, prev, s, pixels=None, capacity=None, samples=None):
    """(out uint32 [capacity], count, samples): `samples` (int32, one per pixel, or None) comes back as a stamped copy."""
    acc, prv = np.asarray(accum, F).reshape(-1, 3), np.asarray(prev, F).reshape(-1, 3)
    npix = len(acc)
    seq = np.arange(npix, dtype=np.int64) if pixels is None else np.asarray(pixels).reshape(-1).astype(np.int64)
    valid = seq[seq < npix]
    if samples is not None:
        samples = np.array(samples, np.int32)
        samples.reshape(-1)[valid] = s.samplesDone
    chosen = valid[selected(acc[valid], prv[valid], s)]
    capacity = len(seq) if capacity is None else capacity
    out = np.full(capacity, SENTINEL, np.uint32)
    kept = min(len(chosen), capacity)
    out[:kept] = chosen[:kept]
    return out, len(chosen), samples


# ---- designed value sets: name -> (desc, accum [n, 3], prev [n, 3]) -------------------------------------------------------
def _ulps(x, k):
    """the float32 k steps above (k < 0: below) x"""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, INF if k > 0 else -INF, dtype=F)
    return x


def designed_sets():
    sets = {}

    def add(name, s, rows):
        a = np.array([r[0] for r in rows], F).reshape(-1, 3)
        p = np.array([r[1] for r in rows], F).reshape(-1, 3)
        sets[name] = (s, a, p)

    zero = (0, 0, 0)
    # d = 2 (d * d = 4), l + floor = 2 + 2 = 4: equality at threshold 1 is not selected; the threshold's, the floor's and
    # one accumulator component's two float32 neighbours on either side
    for k in (-2, -1, 0, 1, 2):
        add(f"equality_threshold{k:+d}", desc(1, 1, 1, 2, _ulps(1, k)), [((1, 1, 0), zero)])
        add(f"equality_floor{k:+d}", desc(1, 1, 1, _ulps(2, k), 1), [((1, 1, 0), zero)])
        # (A_x moves d and l together: e_x = A_x, l = A_x + 1)
        add(f"equality_accum{k:+d}", desc(1, 1, 1, 2, 1), [((_ulps(1, k), 1, 0), zero)])
    # the same equality reached through the weights: A (0.5, 0.5, 0) * 4 - P (0.25, 0.25, 0) * 4 = (1, 1, 0), l = 1 * 2
    add("equality_weighted", desc(4, 4, 2, 2, 1), [((0.5, 0.5, 0), (0.25, 0.25, 0))])
    base_a, base_p = (0.5, 0.25, 0.75), (0.1, 0.2, 0.3)
    rows = []
    for c in range(3):
        a, p = list(base_a), list(base_p)
        a[c] = NAN
        rows.append((a, base_p))
        p[c] = NAN
        rows.append((base_a, p))
    add("nan_inputs", desc(2, 3, 1, 0.01, 0.001), rows + [(base_a, base_p)])  # (the last row: the same values without a NaN)
    add("inf_minus_inf", desc(1, 1, 1, 0.01, 0.001), [((INF, 0, 0), (INF, 0, 0)), ((1, INF, 0), (0, INF, 0)),
                                                        ((-INF, 0, 0), (-INF, 0, 0)), ((INF, 0, 0), (0, 0, 0)),
                                                        ((INF, -INF, 0), zero)])
    # d * d overflows to inf: selected against a finite right side, not against an infinite one
    add("dd_overflow", desc(1, 1, 1, 0, 1), [((1e30, 0, 0), zero), ((3e38, 0, 0), zero), ((1e20, 1e20, 1e20), zero)])
    add("dd_overflow_threshold_inf", desc(1, 1, 1, 0, INF), [((1e30, 0, 0), zero), ((3e38, 0, 0), zero)])
    add("dd_overflow_level_overflow", desc(1, 1, 3e38, 0, 1), [((1e30, 0, 0), zero), ((1e30, 0, 0), (1e30, 0, 0))])
    # l + floor negative: 0 > a negative number; -0: 0 > -0 is false
    add("level_negative", desc(1, 1, 1, 0, 1), [((-1, -1, -1), (-1, -1, -1)), ((-1, -1, -1), zero), ((1, -3, 1), (1, -3, 1))])
    add("level_negative_floor", desc(1, 1, 1, -5, 1), [((1, 1, 1), (1, 1, 1)), ((1, 1, 1), zero), ((2, 2, 2), (0, 0, 0))])
    add("level_minus_zero", desc(1, 1, 1, -0.0, 1), [((-0.0, -0.0, -0.0), (-0.0, -0.0, -0.0)), ((-0.0, -0.0, -0.0), zero),
                                                      (zero, zero)])
    add("level_minus_zero_threshold_negative", desc(1, 1, 1, -0.0, -1), [((-0.0, -0.0, -0.0), zero), (zero, zero)])
    # subnormal products: each row's outcome changes if a subnormal is flushed to zero
    add("subnormal_right_side", desc(1, 1, 1e-10, 0, -1), [((1e-30, 0, 0), (1e-30, 0, 0)), ((1e-30, 1e-30, 1e-30), (1e-30, 1e-30, 1e-30))])
    add("subnormal_both_sides", desc(1, 1, 1e-3, 0, 1e-20), [((1e-22, 0, 0), zero), ((1e-25, 0, 0), zero), ((3e-23, 0, 0), zero)])
    add("subnormal_products", desc(1e-10, 1e-10, 1, 0, -1), [((1e-30, 0, 0), zero), ((1e-30, 0, 0), (2e-30, 0, 0)),
                                                             ((1e-30, 2e-30, 3e-30), (3e-30, 2e-30, 1e-30))])
    add("subnormal_inputs", desc(1, 1, 1, 0, 0), [((1e-40, 0, 0), zero), ((1e-40, 0, 0), (1e-40, 0, 0)), ((1e-45, 0, 0), (0, 0, 1e-45))])
    add("subnormal_floor", desc(1, 1, 1, 1e-40, -1), [(zero, zero), ((0, 0, 0), (1, 0, 0))])
    rows = [(base_a, base_p), (base_a, base_a), (zero, zero), ((-1, -1, -1), zero), ((INF, 0, 0), zero)]
    for name, t in (("nan", NAN), ("zero", 0), ("minus_zero", -0.0), ("inf", INF), ("minus_inf", -INF)):
        add(f"threshold_{name}", desc(1, 1, 1, 0.5, t), rows)
        add(f"threshold_{name}_floor_zero", desc(1, 1, 1, 0, t), rows)
    for s, a, p in sets.values():
        a.setflags(write=False)
        p.setflags(write=False)
    return sets


def random_frame(seed, npix, share=0.5):
    """(desc, accum [npix, 3], prev [npix, 3]): a seeded frame of which about `share` is selected -- prev is accum scaled
    to an earlier sample count and disturbed; a few pixels are black, equal to their snapshot, or NaN."""
    r = np.random.RandomState(seed)
    acc = (r.rand(npix, 3) * r.choice([0.02, 0.3, 1.0, 4.0], (npix, 1))).astype(F)
    prev = (acc * F(0.5) * (1 + (r.rand(npix, 3) - 0.5) * r.choice([0.0, 0.05, 0.5], (npix, 1)))).astype(F)
    odd = r.rand(npix)
    acc[odd < 0.02] = 0
    prev[(odd >= 0.02) & (odd < 0.04)] = 0
    acc[(odd >= 0.04) & (odd < 0.05), r.randint(3)] = NAN
    s = frame_desc(64, 16, 32, 1.0, 0.01)
    with np.errstate(all="ignore"):
        e = np.abs(acc * s.wAccum - prev * s.wPrev).astype(np.float64)
        ratio = e.sum(1) ** 2 / (acc.astype(np.float64).sum(1) * s.wLevel + s.floor)
    s.threshold = F(np.nanquantile(ratio, 1 - share))
    return s, acc, prev


# ---- a whole adaptive frame on the CPU reference -------------------------------------------------------------------------
# name -> (scene, W, H, spp, maxBounce, passes, threshold, floor, capacity, truncating capacity).  threshold, floor and the
# capacities were chosen from the selection sizes this module computes from tests/pixel_pass_reference.py (printed and
# asserted by tests/test_select_reference.py): the first selection non-empty and at most half the frame, a later one a
# non-empty strict subset of its predecessor, the roomy capacity above every count and the truncating one below the first.
ADAPTIVE_FRAMES = {
    "ultracomplex": ("ultracomplex", 64, 40, 12, 4, (3, 3, 2, 2, 2), 0.05, 0.02, 128, 20),      # counts 54, 38, 31, 21
    "box_diffuse_T": ("box_diffuse_T", 64, 40, 12, 4, (3, 3, 2, 2, 2), 0.5, 0.02, 1024, 300),  # counts 683, 203, 70, 31
}


def frame_geometry(name):
    """(triangles, spheres, Scene, camera, trianglesOnly) of an ADAPTIVE_FRAMES scene"""
    import progressive_reference as pr
    import raytracingc_amd as rt
    from chain_path_scenes import SCENES as PATH_SCENES

    if name in PATH_SCENES:
        return PATH_SCENES[name][0], None, rt.default_scene(), PATH_SCENES[name][1], 1
    return pr.geometry(name)


def adaptive_frame(acc_k, spp, passes, threshold, floor, capacity):
    """The frame DeviceScene.render_adaptive_device leaves, from pixel_pass_reference.per_sample's accumulators acc_k
    [spp + 1, pixels, 3] (a pixel's accumulator is a function of its own sample count): (lists, counts, samples, accum)
    -- lists[k - 1] and counts[k - 1] are what the select after pass k >= 1 gives (every list cut at `capacity`)."""
    n = acc_k.shape[1]
    every = np.arange(n)
    samples = np.full(n, passes[0] + passes[1], np.int32)
    prev, acc = acc_k[passes[0], every], acc_k[samples, every]
    done = passes[0] + passes[1]
    out, count, samples = select(acc, prev, frame_desc(spp, passes[0], done, threshold, floor), None, capacity, samples)
    lists, counts = [out], [count]
    for c in passes[2:]:
        before, done = done, done + c
        lst = lists[-1]
        live = lst[lst < n].astype(np.int64)
        assert len(np.unique(live)) == len(live) and (samples[live] == before).all()
        prev = acc
        samples = samples.copy()
        samples[live] += c
        acc = acc_k[samples, every]
        out, count, samples = select(acc, prev, frame_desc(spp, before, done, threshold, floor), lst, capacity, samples)
        lists.append(out)
        counts.append(count)
    return lists, counts, samples, acc
