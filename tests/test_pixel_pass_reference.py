"""tests/pixel_pass_reference.py is right, and the lists of tests/test_gpu_render_pixels.py are not sky alone (CPU only).

Right: the buffers Frame merges from progressive_reference.chain's states for a sequence of whole and pixel passes equal an
independent computation -- progressive_reference.sample run on the listed rays alone, from the state the frame holds for
them, with main.c:99's float32 arithmetic -- in accumulator words, RNG states, Color bytes and calculateRayCollision calls;
the pixels that are not listed keep their bytes; and whole passes alone end as oracle.render's frame.

Not sky alone: on every scene the GPU test uses a mixed list on (64x40, spp 12, maxBounce 4), every mixed list of at least
24 pixels holds at least 8 pixels of each class -- pixels that never hit, pixels that hit but never more than once in a
sample, pixels with two or more hits in some sample -- or, where the whole frame has fewer than 8 of a class, all of them,
and in every case at least half of the list hits.  Two frames are short of a class, and the test says which (the counts are
printed): the reference's default box is closed -- every primary ray hits and every path bounces again, as
tests/test_progressive_reference.py asserts -- so the first two classes are empty there; and ultracomplex is so open that
at maxBounce 4 a single pixel of the frame ever hits twice in a sample (that one is in every list, lists of one included).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle.binding as orc
import pixel_pass_reference as ppr
import progressive_reference as pr
from raytracingc_amd._abi import RtcRenderDesc

W, H, SPP, MAX_BOUNCE = 64, 40, 12, 4
SCENES = pr.SCENE_NAMES + ("chunks_open5",)   # the scenes of the GPU test's equivalence cases
CLOSED = ("default",)
LIST_SIZES = (1, 63, 64, 65, 129)
F = np.float32


def _desc(name, row_start=0, stride=1, band=0, w=W, h=H):
    return RtcRenderDesc(w, h, SPP, MAX_BOUNCE, pr.geometry(name)[4], row_start, stride, 0, band)


@functools.lru_cache(maxsize=None)
def _states(name):
    tris, sph, scene, cam, _ = pr.geometry(name)
    cache = {}
    d = _desc(name)
    return ppr.per_sample(tris, sph, scene, cam, d, cache), ppr.classes(pr.hits_per_sample(tris, sph, scene, cam, d, cache))


def _independent(name, d, pixels, acc, rng, count):
    """`count` iterations of main.c:98-99 for the listed pixels alone, from (acc, rng): progressive_reference.sample on
    their rays, no cache, no chain."""
    tris, sph, scene, cam, _ = pr.geometry(name)
    rays = pr.launch_rays(cam, pr._launch(d))[pixels]
    acc, rng, calls = np.array(acc, F), np.array(rng, np.uint32), 0
    w = F(1.0 / np.float64(d.spp))
    with np.errstate(all="ignore"):
        for _ in range(count):
            rad, rng, c, _ = pr.sample(tris, sph, scene, d, rays, rng)
            acc = (acc + (rad * w).astype(F)).astype(F)
            calls += int(c.sum())
    return acc, rng, calls


@pytest.mark.parametrize("name", SCENES)
def test_mixed_lists_hold_every_class(name):
    _, cls = _states(name)
    print(f"{name}: {[len(c) for c in cls]} pixels never hit / hit once at most / hit twice or more in some sample")
    assert sum(len(c) for c in cls) == W * H
    for n in LIST_SIZES + (24, 25, 26):
        lst = ppr.mixed_list(cls, n)
        assert len(lst) == n and len(np.unique(lst)) == n and lst.dtype == np.uint32
        assert not np.array_equal(lst, np.sort(lst)) or n == 1, "shuffled"
        counts = ppr.class_counts(cls, lst)
        assert sum(counts) == n
        if n < 24:
            continue
        assert all(c >= min(8, len(k)) for c, k in zip(counts, cls)), (name, n, counts)
        assert counts[1] + counts[2] >= n // 2, (name, n, counts)
    short = [ppr.CLASS_NAMES[i] for i in range(3) if len(cls[i]) < 8]
    assert short == {"default": ["never", "single"], "ultracomplex": ["several"]}.get(name, []), (name, short)
    assert len(cls[2]) >= 1
    assert ppr.mixed_list(cls, 1)[0] in cls[2], "a list of one pixel is a pixel with several hits"
    every = ppr.every_pixel(W * H)
    assert np.array_equal(np.sort(every), np.arange(W * H)) and not np.array_equal(every, np.arange(W * H))


@pytest.mark.parametrize("name", SCENES)
def test_merged_passes_equal_the_listed_rays_alone(name):
    """Whole [0, 5), a pixel pass [5, 12) over a mixed list, against the independent computation; then a fresh pixel pass
    [0, 12) over another list on poisoned buffers."""
    states, cls = _states(name)
    d = _desc(name)
    fr = ppr.Frame(states)
    whole_calls = fr.whole_pass(0, 5)
    assert whole_calls == int(states[3][:5].sum())
    before = fr.buffers()
    lst = ppr.mixed_list(cls, 65).astype(np.int64)
    stale = np.concatenate([lst[:30], [W * H, W * H + 63, 0xFFFFFFFF], lst[30:]])  # out-of-range indices are skipped
    calls = fr.pixel_pass(5, 7, stale)
    acc, rng, col = fr.buffers()
    iacc, irng, icalls = _independent(name, d, lst, before[0].view(F)[lst], before[1][lst], 7)
    assert np.array_equal(acc[lst], iacc.view(np.uint32)) and np.array_equal(rng[lst], irng) and calls == icalls
    assert np.array_equal(col[lst], pr.to_color(iacc))
    rest = np.setdiff1d(np.arange(W * H), lst)
    for got, was in zip((acc, rng, col), before):
        assert np.array_equal(got[rest], was[rest])
    assert np.array_equal(fr.samples[lst], np.full(65, 12)) and (fr.samples[rest] == 5).all()
    # the listed pixels are the finished frame's
    tris, sph, scene, cam, _ = pr.geometry(name)
    ocol, oacc, _ = orc.render(tris, sph, scene, cam, d, threads=8)
    assert np.array_equal(acc[lst], oacc.reshape(-1, 3).view(np.uint32)[lst]) and np.array_equal(col[lst], ocol.reshape(-1, 3)[lst])

    fresh = ppr.Frame(states)
    calls = fresh.pixel_pass(0, 12, lst)
    acc, rng, col = fresh.buffers()
    iacc, irng, icalls = _independent(name, d, lst, np.zeros((65, 3), F), pr.seeds(d)[lst], 12)
    assert np.array_equal(acc[lst], iacc.view(np.uint32)) and np.array_equal(rng[lst], irng) and calls == icalls
    assert (acc[rest] == 0xFFFFFFFF).all() and (rng[rest] == 0xFFFFFFFF).all() and (col[rest] == 0xFF).all()
    sky = np.intersect1d(lst, cls[0])
    assert np.array_equal(rng[sky], pr.seeds(d)[sky]), "a listed pixel that never hits holds its seed"


def test_whole_passes_alone_end_as_the_oracle_and_passes_alternate():
    name = "fsuzane"
    states, cls = _states(name)
    tris, sph, scene, cam, _ = pr.geometry(name)
    d = _desc(name)
    ocol, oacc, oseg = orc.render(tris, sph, scene, cam, d, threads=8)
    fr = ppr.Frame(states)
    assert fr.whole_pass(0, 5) + fr.whole_pass(5, 7) == oseg
    acc, rng, col = fr.buffers()
    assert np.array_equal(acc, oacc.reshape(-1, 3).view(np.uint32)) and np.array_equal(col, ocol.reshape(-1, 3))
    # whole [0, 3), every pixel [3, 5) as a list, whole [5, 12): the same frame
    fr2 = ppr.Frame(states)
    total = fr2.whole_pass(0, 3) + fr2.pixel_pass(3, 2, ppr.every_pixel(W * H)) + fr2.whole_pass(5, 7)
    assert total == oseg and all(np.array_equal(a, b) for a, b in zip(fr2.buffers(), (acc, rng, col)))
    # an adaptive frame: three shrinking selections
    fr3 = ppr.Frame(states)
    fr3.whole_pass(0, 3)
    sel = ppr.mixed_list(cls, 129).astype(np.int64)
    for k, (first, count) in enumerate(((3, 4), (7, 3), (10, 2))):
        sel = sel[: len(sel) // (k + 1)]
        fr3.pixel_pass(first, count, sel)
    assert sorted(np.unique(fr3.samples).tolist()) == [3, 7, 10, 12]
    a3, r3, _ = fr3.buffers()
    for k in (3, 7, 10, 12):
        who = np.flatnonzero(fr3.samples == k)
        assert np.array_equal(a3[who], states[0][k, who].view(np.uint32)) and np.array_equal(r3[who], states[1][k, who])
    with pytest.raises(AssertionError):
        fr3.whole_pass(12, 1)  # not every pixel is at 12
