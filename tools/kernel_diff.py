#!/usr/bin/env python3
"""Compare the device code of the library's HIP translation units between two source trees, kernel by kernel, and list the
resource use of the kernels only the second has.

    tools/kernel_diff.py [--may-differ REGEX] OLD_TREE NEW_TREE

Each raytracingc_amd/csrc/*.hip of NEW_TREE (rtc_render.hip first; a unit OLD_TREE lacks has only new kernels) is
compiled in both trees for gfx950 with the Makefile's flags to assembly
(--cuda-device-only -S, with -Rpass-analysis=kernel-resource-usage).  A kernel's text is the lines between its label and
its .Lfunc_end; local labels (.LBB<function>_<block>) are renumbered by the function's own order, so a kernel that moved
in the file still compares equal.  A template parameter added at the END of a kernel template's list with the default
`false` changes the mangled names of the existing instantiations and nothing else: such names of NEW are matched with
OLD's by dropping trailing `Lb0E` arguments.  The order of emission is compared too: NEW must emit OLD's kernels first,
in OLD's order (the non-template kernels in source order, then the templates' instantiations in the order of the explicit
instantiation list at the end of rtc_render.hip, where new ones are appended).  Exit status 1 when a kernel of OLD is
missing from NEW or differs, or when that order changed.  Needs only hipcc (no GPU).

--may-differ REGEX names kernels (a search on the mangled symbol) that are held to their resources instead of their
instructions: for each, OLD's and NEW's line count, VGPRs, SGPRs, spills, scratch, LDS and waves per SIMD are printed, and
it fails only when missing or when NEW has more VGPRs, any scratch, any VGPR spill, more LDS or fewer waves per SIMD than
OLD (SGPRs and SGPR spills are reported, not judged).  Every kernel not named must still be `same`, and the order kept."""
from __future__ import annotations

import argparse
import glob
import os
import re
import subprocess
import sys

FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-std=c++17",
         "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", "-"]


def compile_tree(tree, unit="rtc_render.hip"):
    src = f"{tree}/raytracingc_amd/csrc/{unit}"
    if not os.path.exists(src):
        return "", ""
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, src], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    return r.stdout, r.stderr


def kernels(asm):
    """{kernel symbol: its normalised text}, for every .amdhsa_kernel of the module."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M))
    out, cur, body = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in names:
            cur, body = m.group(1), []
            continue
        if cur and line.startswith(".Lfunc_end"):
            text = "\n".join(body)
            fn = re.search(r"\.LBB(\d+)_", text)
            if fn:
                text = re.sub(r"\.LBB%s_" % fn.group(1), ".LBBf_", text)
            out[cur], cur = text.replace(cur, "KERNEL"), None  # (its descriptor, before .Lfunc_end, names it)
            continue
        if cur is not None:
            s = line.split(";")[0].rstrip()  # (comments carry the source tree's paths and offsets)
            if s.strip() and not s.lstrip().startswith((".loc", ".file", ".cfi")):
                body.append(s)
    return out


def resources(remarks):
    rows, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: [^:]*?\s{2,}([A-Za-z /\[\]]+): (\d+)", line)
        if cur is not None and m:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows


def demangle(names):
    if not names:  # (c++filt without arguments would read its standard input)
        return {}
    try:
        r = subprocess.run(["c++filt", *names], capture_output=True, text=True)
    except OSError:
        return {n: n for n in names}
    return dict(zip(names, r.stdout.splitlines())) if r.returncode == 0 and names else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--may-differ", metavar="REGEX", help="kernels held to their resources, not their instructions")
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    a = ap.parse_args()
    may_differ = re.compile(a.may_differ) if a.may_differ else None
    units = sorted((os.path.basename(f) for f in glob.glob(f"{a.new_tree}/raytracingc_amd/csrc/*.hip")),
                   key=lambda u: (u != "rtc_render.hip", u))
    bad = 0
    for unit in units:
        print(f"==== {unit}")
        bad += diff_unit(a.old_tree, a.new_tree, unit, may_differ)
        print()
    sys.exit(1 if bad else 0)


# the resource remarks a kernel that may differ is held to and reported by: (remark, short name, what fails it)
HELD = [("VGPRs", "VGPRs", lambda o, n: n > o), ("TotalSGPRs", "SGPRs", None), ("SGPRs Spill", "SGPR spills", None),
        ("VGPRs Spill", "VGPR spills", lambda o, n: n > 0), ("ScratchSize [bytes/lane]", "scratch", lambda o, n: n > 0),
        ("LDS Size [bytes/block]", "LDS", lambda o, n: n > o), ("Occupancy [waves/SIMD]", "waves/SIMD", lambda o, n: n < o)]


def held_to_resources(old_lines, new_lines, o, n):
    """The report of one kernel that may differ, and whether its resources fail it (a remark that is missing does)."""
    cells, worse = [f"lines {old_lines} -> {new_lines}"], []
    for key, name, fails in HELD:
        ov, nv = ((r.get(key, r.get("SGPRs")) if key == "TotalSGPRs" else r.get(key)) for r in (o, n))
        cells.append(f"{name} {ov} -> {nv}")
        if fails and (ov is None or nv is None or fails(ov, nv)):
            worse.append(name)
    return ", ".join(cells), worse


def diff_unit(old_tree, new_tree, unit, may_differ=None):
    old_asm, old_rem = compile_tree(old_tree, unit)
    new_asm, new_rem = compile_tree(new_tree, unit)
    old, new = kernels(old_asm), kernels(new_asm)
    by_old_name = {}
    for n in new:
        k = n
        while k not in old and "Lb0EEv" in k:  # ...Lb0E + E (the list's end) + v: drop the last argument
            k = k.replace("Lb0EEv", "Ev", 1)
        by_old_name[k if k in old else n] = n
    bad = held = 0
    old_res, res = resources(old_rem), resources(new_rem)
    for k in sorted(old):
        n = by_old_name.get(k)
        verdict = "MISSING" if n is None else ("same" if old[k] == new[n] else "DIFFERS")
        report = None
        if verdict == "DIFFERS" and may_differ and may_differ.search(k):
            report, worse = held_to_resources(len(old[k].splitlines()), len(new[n].splitlines()), old_res.get(k, {}),
                                              res.get(n, {}))
            verdict = "WORSE" if worse else "differs"
            held += 1
            report += f"  ({'WORSE: ' + ', '.join(worse) if worse else 'held to its resources: no worse'})"
        bad += verdict not in ("same", "differs")
        print(f"{verdict:8s} {len(old[k].splitlines()):6d} lines  {k}" + (f"  (now {n})" if n and n != k else ""))
        if report:
            print(f"           {report}")
    # the order of emission: OLD's kernels in OLD's order, then the new ones (so OLD's keep their relative offsets)
    to_old = {n: k for k, n in by_old_name.items()}
    seq = [to_old[n] for n in new]
    kept = [k for k in seq if k in old]
    in_order = kept == [k for k in old if k in kept] and all(k in old for k in seq[:len(kept)])
    print(f"\nemission order: {'the existing kernels first, in their order' if in_order else 'CHANGED'}")
    if not in_order:
        print("  was: " + " ".join(old) + "\n  now: " + " ".join(new))
    bad += not in_order
    added = sorted(n for k, n in by_old_name.items() if k not in old)
    dm = demangle(added)
    print(f"\n{len(old)} kernels compared, {bad} changed or missing" +
          (f", {held} held to their resources" if may_differ else "") + f"; {len(added)} new:")
    for n in added:
        r = res.get(n, {})
        print(f"  {dm[n]}: VGPRs {r.get('VGPRs')}, SGPRs {r.get('TotalSGPRs', r.get('SGPRs'))}, scratch {r.get('ScratchSize [bytes/lane]')} B/lane, "
              f"spills {r.get('SGPRs Spill')} SGPR / {r.get('VGPRs Spill')} VGPR, waves/SIMD "
              f"{r.get('Occupancy [waves/SIMD]')}, LDS {r.get('LDS Size [bytes/block]')} B")
    return bad


if __name__ == "__main__":
    main()
