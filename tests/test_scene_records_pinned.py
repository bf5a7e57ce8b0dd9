"""The host scene records, pinned: every record array rtc_scene_records_host builds, and rtc_regroup_membership_host's
membership, hash to what the commit before rtc_records.h built (tests/golden/scene_records_sha256.json, made by
tests/golden/make_scene_records.py from that commit).  The GPU tests hold the device equal to the host byte for byte
(tests/test_gpu_scene_update.py, tests/test_gpu_regroup.py); this holds the host equal to a fixed value, so a change to the
shared arithmetic (rtc_records.h, rtc_regroup.h) that moves a byte -- a NaN's payload and a zero's sign included -- fails
here without a GPU.  No reference counterpart (main.c:229-243 builds flat arrays once)."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

import raytracingc_amd as rt
from conftest import GOLDEN
from scene_record_cases import CASES, digests

with open(os.path.join(GOLDEN, "scene_records_sha256.json")) as f:
    PINNED = json.load(f)


def test_every_case_is_pinned():
    assert sorted(PINNED) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_records_hash_to_the_pinned_ones(case):
    got = digests(rt, case)
    assert sorted(got) == sorted(PINNED[case])
    for what, want in PINNED[case].items():
        differ = [name for name in want if got[what].get(name) != want[name]]
        assert not differ and sorted(got[what]) == sorted(want), f"{case} {what}: {differ} differ from the pinned bytes"


def test_record_arrays_are_the_librarys_table():
    """RECORD_ARRAYS and the dwords per record are the library's table (rtc_layout.h kSceneArrays), seen through the sizes
    rtc_scene_records_host reports: six arrays, of 9 triangles and 2 spheres -> 24, 24, 2, 16, 2 and 1 records."""
    t = np.zeros(9, rt.TRIANGLE_DT)
    s = np.zeros(2, rt.SPHERE_DT)
    sizes = (C.c_size_t * 7)(*([0] * 6), 12345)
    args = (t.ctypes.data_as(C.c_void_p), 9, None, s.ctypes.data_as(C.c_void_p), 2, *([None] * 6))
    assert rt.lib().rtc_scene_records_host(*args, sizes) == 0
    assert sizes[6] == 12345  # (six sizes and no more)
    assert len(rt.RECORD_ARRAYS) == 6 == len(rt._RECORD_WORDS)
    records = dict(tris=24, mats=24, spheres=2, clTris=16, clusters=2, chunks=1)
    assert tuple(records) == tuple(rt.RECORD_ARRAYS)
    assert [sizes[k] for k in range(6)] == [records[n] * 4 * w for n, w in zip(rt.RECORD_ARRAYS, rt._RECORD_WORDS)]
