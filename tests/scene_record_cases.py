"""The cases whose host scene records are pinned by hash (tests/golden/scene_records_sha256.json, written once by
tests/golden/make_scene_records.py from the commit before the records' arithmetic was stated once in rtc_records.h;
tests/test_scene_records_pinned.py rebuilds them).  Per case: the SHA-256 of each of the six record arrays' bytes as
rtc_scene_records_host returns them and of rtc_regroup_membership_host's result, for the upload's build and, for every
helper of moving_scenes.HELPERS, for the refit to the moved triangles.  Bytes, not values: NaN payloads and the signs of
zeros count.  No reference counterpart (main.c:229-243 builds flat arrays once)."""
from __future__ import annotations

import hashlib

import numpy as np

from adversarial_scenes import SCENES as ADVERSARIAL
from conftest import load_tris
from material_scenes import SPHERE_NAMES, sphere_scene
from moving_scenes import HELPERS, synthetic

MODELS = ("cube", "ultracomplex", "suzannes")  # suzannes: several chunks
SYNTHETIC = (1, 7, 8, 9, 255, 256, 257, 264)  # a partial last cluster, exactly one chunk, a second chunk of one cluster
assert len(ADVERSARIAL) == 29

CASES = ([f"model_{m}" for m in MODELS] + [f"n{n}" for n in SYNTHETIC] + [f"adversarial_{a}" for a in sorted(ADVERSARIAL)]
         + list(SPHERE_NAMES))


def scene(case):
    """(triangles, spheres or None) of a case."""
    if case.startswith("model_"):
        return load_tris(case[len("model_"):])[0], None
    if case.startswith("adversarial_"):
        return ADVERSARIAL[case[len("adversarial_"):]][0], None
    if case in SPHERE_NAMES:
        return sphere_scene(case)[:2]
    return synthetic(int(case[1:])), None


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(rt, case):
    """{"upload" | helper: {array name | "membership": sha256}} of a case, computed with the package `rt`."""
    tris, spheres = scene(case)
    out = {}
    for what in ("upload", *sorted(HELPERS)):
        moved = None if what == "upload" else HELPERS[what](tris)
        rec = rt.scene_records_host(tris, moved, spheres)
        assert tuple(rec) == tuple(rt.RECORD_ARRAYS) and len(rec) == 6
        out[what] = {name: _sha(a) for name, a in rec.items()}
        out[what]["membership"] = _sha(rt.regroup_membership_host(tris if moved is None else moved))
    return out
