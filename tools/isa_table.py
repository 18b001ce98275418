#!/usr/bin/env python3
"""Register / spill / scratch figures of every kernel of a built library, from the gfx950 code object's metadata note, and the
comparison of two builds (the gate of a change that must leave the existing kernels' allocation alone).

    python tools/isa_table.py robosumo_selfplay_amd/csrc/libsumo_hip.so                       # table of one library
    python tools/isa_table.py <parent>/libsumo_hip.so robosumo_selfplay_amd/csrc/libsumo_hip.so    # + comparison, exit 1 on a difference

    python tools/isa_table.py --only sumo_ <parent>/libsumo_hip.so robosumo_selfplay_amd/csrc/libsumo_hip.so   # the project's own kernels

Kernels present in both libraries must agree in every figure; kernels only in the second one are listed as new."""
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from robosumo_selfplay_amd.codegen_check import LLVM, code_objects  # noqa: E402

FIELDS = (".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size")


def table(lib):
    # every code object of the library: build.py links sumo_engine.hip from several translation units, each with its own
    notes = "\n".join(subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True) for co in code_objects(lib))
    out, cur = {}, {}
    for ln in notes.splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(.*)$", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- .") and cur.get(".symbol"):      # next entry of amdhsa.kernels
            out[cur[".symbol"]] = cur
            cur = {}
        if m.group(1) in FIELDS + (".symbol",):
            cur[m.group(1)] = m.group(2).strip().strip("'")
    if cur.get(".symbol"):
        out[cur[".symbol"]] = cur
    filt = shutil.which("c++filt") or os.path.join(LLVM, "llvm-cxxfilt")
    demangle = subprocess.run([filt], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    return {name.replace(".kd", ""): tuple(int(out[sym].get(f, -1)) for f in FIELDS) for sym, name in zip(out, demangle)}


def fmt(t):
    return "\n".join("%-110s %s" % (k[:110], " ".join("%5d" % v for v in t[k])) for k in sorted(t))


def main(argv):
    only = None
    if "--only" in argv:                                  # --only sumo_ : the kernels whose demangled name contains the text
        k = argv.index("--only")
        only, argv = argv[k + 1], argv[:k] + argv[k + 2:]
    head = "%-110s %s" % ("kernel", " ".join(f.strip(".").replace("_count", "").replace("private_segment_fixed_size", "scratch") for f in FIELDS))
    tabs = [table(p) for p in argv]
    if only:
        tabs = [{k: v for k, v in t.items() if only in k} for t in tabs]
    for p, t in zip(argv, tabs):
        print("== %s (%d kernels)\n%s\n%s\n" % (p, len(t), head, fmt(t)))
    if len(tabs) == 2:
        a, b = tabs
        diff = [k for k in a if k in b and a[k] != b[k]]
        gone = [k for k in a if k not in b]
        print("== comparison: %d common kernels, %d differ, %d missing in the second, %d new" % (len(set(a) & set(b)), len(diff), len(gone),
                                                                                              len(set(b) - set(a))))
        for k in diff:
            print("DIFF %s: %s -> %s" % (k, a[k], b[k]))
        for k in gone:
            print("MISSING %s" % k)
        for k in sorted(set(b) - set(a)):
            print("NEW  %s" % k)
        return 1 if diff or gone else 0
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
