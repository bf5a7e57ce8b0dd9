#!/usr/bin/env python3
"""Writes tests/golden/scene_records_sha256.json: the hashes of the host scene records of tests/scene_record_cases.py.

    python tests/golden/make_scene_records.py BUILT_TREE

BUILT_TREE is a built checkout of the commit whose records are to be pinned; the package is imported from it, the cases
from this tree.  The committed fixture was made once from the commit before rtc_records.h; it is never regenerated
from the tree under test (tests/test_scene_records_pinned.py would then compare the tree with itself)."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    tree = os.path.abspath(sys.argv[1])
    sys.path.insert(0, tree)
    import raytracingc_amd as rt

    assert os.path.dirname(os.path.dirname(os.path.abspath(rt.__file__))) == tree, rt.__file__
    sys.path.insert(1, os.path.dirname(HERE))
    import scene_record_cases as cases

    assert sys.modules["raytracingc_amd"] is rt
    out = {case: cases.digests(rt, case) for case in cases.CASES}
    with open(os.path.join(HERE, "scene_records_sha256.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases from {tree}")


if __name__ == "__main__":
    main()
