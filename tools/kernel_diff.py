#!/usr/bin/env python3
"""Compare the device code of the library's HIP translation units between two source trees, kernel by kernel, and list the
resource use of the kernels only the second has.

    tools/kernel_diff.py OLD_TREE NEW_TREE

Each raytracingc_amd/csrc/*.hip of NEW_TREE (rtc_render.hip first; a unit OLD_TREE lacks has only new kernels) is
compiled in both trees for gfx950 with the Makefile's flags to assembly
(--cuda-device-only -S, with -Rpass-analysis=kernel-resource-usage).  A kernel's text is the lines between its label and
its .Lfunc_end; local labels (.LBB<function>_<block>) are renumbered by the function's own order, so a kernel that moved
in the file still compares equal.  A template parameter added at the END of a kernel template's list with the default
`false` changes the mangled names of the existing instantiations and nothing else: such names of NEW are matched with
OLD's by dropping trailing `Lb0E` arguments.  The order of emission is compared too: NEW must emit OLD's kernels first,
in OLD's order (the non-template kernels in source order, then the templates' instantiations in the order of the explicit
instantiation list at the end of rtc_render.hip, where new ones are appended).  Exit status 1 when a kernel of OLD is
missing from NEW or differs, or when that order changed.  Needs only hipcc (no GPU)."""
from __future__ import annotations

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
    units = sorted((os.path.basename(f) for f in glob.glob(f"{sys.argv[2]}/raytracingc_amd/csrc/*.hip")),
                   key=lambda u: (u != "rtc_render.hip", u))
    bad = 0
    for unit in units:
        print(f"==== {unit}")
        bad += diff_unit(unit)
        print()
    sys.exit(1 if bad else 0)


def diff_unit(unit):
    old_asm, _ = compile_tree(sys.argv[1], unit)
    new_asm, new_rem = compile_tree(sys.argv[2], unit)
    old, new = kernels(old_asm), kernels(new_asm)
    by_old_name = {}
    for n in new:
        k = n
        while k not in old and "Lb0EEv" in k:  # ...Lb0E + E (the list's end) + v: drop the last argument
            k = k.replace("Lb0EEv", "Ev", 1)
        by_old_name[k if k in old else n] = n
    bad = 0
    for k in sorted(old):
        n = by_old_name.get(k)
        verdict = "MISSING" if n is None else ("same" if old[k] == new[n] else "DIFFERS")
        bad += verdict != "same"
        print(f"{verdict:8s} {len(old[k].splitlines()):6d} lines  {k}" + (f"  (now {n})" if n and n != k else ""))
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
    res, dm = resources(new_rem), demangle(added)
    print(f"\n{len(old)} kernels compared, {bad} changed or missing; {len(added)} new:")
    for n in added:
        r = res.get(n, {})
        print(f"  {dm[n]}: VGPRs {r.get('VGPRs')}, SGPRs {r.get('TotalSGPRs', r.get('SGPRs'))}, scratch {r.get('ScratchSize [bytes/lane]')} B/lane, "
              f"spills {r.get('SGPRs Spill')} SGPR / {r.get('VGPRs Spill')} VGPR, waves/SIMD "
              f"{r.get('Occupancy [waves/SIMD]')}, LDS {r.get('LDS Size [bytes/block]')} B")
    return bad


if __name__ == "__main__":
    main()
