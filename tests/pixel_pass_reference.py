"""The expected buffers of a sequence of whole passes and pixel passes of one progressive frame (rtc_render_samples_async
and rtc_render_pixels_async), with no code under test in the loop.

A pixel's state is a function of how many samples it has had: per_sample(...) is progressive_reference.chain over one-sample
passes -- the reference's accumulator, rngState and Color after k = 0 .. spp iterations of main.c:98-99 for every pixel of
the launch -- and Frame merges those states: a whole pass moves every pixel on by `count` samples, a pixel pass the listed
ones, and the Color bytes change only where a pass writes them.  The calculateRayCollision calls of a pass are summed from
progressive_reference.sample's per-pixel calls at the chain's own states.

The lists are built by rule from progressive_reference.hits_per_sample (classes): pixels that never hit, pixels that hit
and never more than once in a sample, pixels with two or more hits in some sample.  mixed_list(classes, n) takes pixels in
raster order from the three classes in turn (several hits first; a class that has run out is passed over) and shuffles
them with a fixed seed.  tests/test_pixel_pass_reference.py checks the helper against progressive_reference.sample run on
the listed rays alone, and that the lists are not sky alone."""
from __future__ import annotations

import numpy as np

import progressive_reference as pr

F = np.float32
CLASS_NAMES = ("never", "single", "several")


def per_sample(tris, spheres, scene, cam, desc, cache=None):
    """(accum float32 [spp + 1, pixels, 3], rng uint32 [spp + 1, pixels], colors uint8 [spp + 1, pixels, 3], calls int64
    [spp, pixels]): the state after k samples, k = 0 the frame's start (+0, the seeds); calls[k] what sample k traced."""
    cache = {} if cache is None else cache
    ch = pr.chain(tris, spheres, scene, cam, desc, [1] * desc.spp, cache)
    n = ch[0][2].size
    acc = np.stack([np.zeros((n, 3), F)] + [c[1].reshape(n, 3) for c in ch])
    rng = np.stack([pr.seeds(desc)] + [c[2].reshape(n) for c in ch])
    col = np.stack([pr.to_color(acc[0])] + [c[3].reshape(n, 3) for c in ch])
    rays = pr.launch_rays(cam, pr._launch(desc))
    calls = np.stack([pr.sample(tris, spheres, scene, desc, rays, rng[k], cache)[2] for k in range(desc.spp)])
    assert [int(c.sum()) for c in calls] == [c[4] for c in ch]
    for a in (acc, rng, col, calls):
        a.setflags(write=False)
    return acc, rng, col, calls


class Frame:
    """The three buffers of a frame whose pixels have had different numbers of samples.  `states`: per_sample's result;
    `fill`: the byte every buffer holds before the first pass (the tests poison them with 0xFF)."""

    def __init__(self, states, fill=0xFF):
        self.acc_k, self.rng_k, self.col_k, self.calls_k = states
        n = self.rng_k.shape[1]
        self.spp = self.calls_k.shape[0]
        self.samples = np.zeros(n, np.int64)
        self.accum = np.full((n, 3), fill * 0x01010101, np.uint32).view(F)
        self.rng = np.full(n, fill * 0x01010101, np.uint32)
        self.colors = np.full((n, 3), fill, np.uint8)
        self.started = np.zeros(n, bool)

    def _advance(self, first, count, who):
        """the pixels `who` (indices) by `count` samples, as a pass with range [first, first + count) has it: with
        first == 0 from the frame's start, else from what the pixel holds.  Returns the pass's calls."""
        if first == 0:
            self.samples[who] = 0
        else:
            assert self.started[who].all(), "a pass with first > 0 over a pixel that holds no state"
        k0 = self.samples[who]
        assert (k0 + count <= self.spp).all()
        k1 = k0 + count
        self.accum[who], self.rng[who], self.colors[who] = self.acc_k[k1, who], self.rng_k[k1, who], self.col_k[k1, who]
        self.samples[who], self.started[who] = k1, True
        return int(sum(self.calls_k[k0 + j, who].sum() for j in range(count)))

    def whole_pass(self, first, count):
        assert first == 0 or (self.samples == first).all(), "a whole pass continues every pixel from the same sample"
        return self._advance(first, count, np.arange(len(self.samples)))

    def pixel_pass(self, first, count, pixels):
        """`pixels`: compact indices; those at or past the frame's pixel count are skipped."""
        p = np.asarray(pixels, np.int64)
        p = p[p < len(self.samples)]
        assert len(np.unique(p)) == len(p), "duplicates are the caller's error"
        return self._advance(first, count, p)

    def buffers(self):
        """(accum as uint32 words [pixels, 3], rng [pixels], colors [pixels, 3]), copies"""
        return self.accum.view(np.uint32).copy(), self.rng.copy(), self.colors.copy()


def classes(hits):
    """progressive_reference.hits_per_sample's [spp, pixels] as three raster-ordered index arrays: never hit, hit but never
    more than once in a sample, two or more hits in some sample."""
    most = hits.max(0)
    return tuple(np.flatnonzero(m) for m in (most == 0, most == 1, most >= 2))


def mixed_list(cls, n, seed=20240917):
    """n pixels (fewer if the frame has fewer): in turn the next pixel, in raster order, of the classes several, single,
    never -- a class that has run out is passed over -- shuffled with a fixed seed.  uint32."""
    order = [cls[2], cls[1], cls[0]]
    take = [0, 0, 0]
    left = n
    while left > 0 and any(take[c] < len(order[c]) for c in range(3)):
        for c in range(3):
            if left > 0 and take[c] < len(order[c]):
                take[c] += 1
                left -= 1
    out = np.concatenate([order[c][:take[c]] for c in range(3)]).astype(np.uint32)
    np.random.RandomState(seed).shuffle(out)
    return out


def every_pixel(n, seed=20240917):
    out = np.arange(n, dtype=np.uint32)
    np.random.RandomState(seed).shuffle(out)
    return out


def class_counts(cls, pixels):
    """how many of `pixels` lie in each class (never, single, several)"""
    return tuple(int(np.isin(pixels, c).sum()) for c in cls)
