#!/usr/bin/env python3
"""Before / after counter for a change that is to leave kernels as they are (profiles/pixel_tile/README.md, profiles/voxel_block/README.md):
compiles kernel units of two source trees to gfx950 assembly with each tree's own Makefile flags (make -pn) and prints (markdown)
  * whether the assembly of the units given with --untouched is byte-identical, and
  * for every kernel of the units given with --edited whose demangled name matches --kernels: registers, scratch, LDS, occupancy (the
    compiler's own kernel info, the figures `make resources` prints), the instruction count and the counts of global loads, global
    stores, global atomics and ds_bpermute.

  tools/kernel_counts.py BEFORE_TREE AFTER_TREE --untouched UNIT,... --edited UNIT,... --kernels REGEX [--work DIR]      (a tree: a checkout's root)

-cuid=0 pins the compile-unit id, which otherwise hashes the source's path into a symbol name.  Needs no GPU.  It asserts on nothing."""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INFO = {"vgpr": r"; NumVgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)", "lds": r"; LDSByteSize: (\d+)", "occ": r"; Occupancy: (\d+)"}
COLS = ["vgpr", "sgpr", "scratch", "lds", "occ", "instr", "gload", "gstore", "gatomic", "bperm"]


def flags_of(tree):
    """CXXFLAGS and HIPFLAGS as the tree's own Makefile sets them"""
    db = subprocess.run(["make", "-pn", "-C", os.path.join(tree, "mcray-tracing_amd")], capture_output=True, text=True).stdout
    return [w for var in ("CXXFLAGS", "HIPFLAGS") for w in re.search(r"^%s :?= (.*)$" % var, db, re.M).group(1).split()]


def compile_unit(tree, unit, out):
    src = os.path.join(tree, "mcray-tracing_amd", "csrc", unit + ".hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950"] + flags_of(tree) + ["--cuda-device-only", "-S", "-cuid=0", "-o", out, src], capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s does not compile:\n%s" % (src, r.stderr))


def kernels_of(path, pattern):
    """{demangled kernel name: counts} of the kernels whose name matches"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:.*?; Kernel info:\n(.*?)\n\s*\.", text, re.M | re.S):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        if not pattern.search(name):
            continue
        ins = [l.split()[0] for l in m.group(2).splitlines() if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
        row = {k: int(re.search(p, m.group(3)).group(1)) for k, p in INFO.items()}
        row.update(instr=len(ins), gload=sum(i.startswith("global_load") for i in ins), gstore=sum(i.startswith("global_store") for i in ins),
                   gatomic=sum(i.startswith("global_atomic") for i in ins), bperm=sum(i == "ds_bpermute_b32" for i in ins))
        out[re.sub(r"^void mcrt::|\(mcrt::\w+\)$", "", name)] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before"); ap.add_argument("after")
    ap.add_argument("--untouched", default="", help="units (csrc/NAME.hip) whose assembly must not differ, comma-separated")
    ap.add_argument("--edited", default="", help="units whose kernels are counted")
    ap.add_argument("--kernels", default=".", help="regular expression a counted kernel's demangled name matches")
    ap.add_argument("--work", default="build/kernel_counts")
    o = ap.parse_args()
    untouched, edited, pattern, work = [u for u in o.untouched.split(",") if u], [u for u in o.edited.split(",") if u], re.compile(o.kernels), o.work
    jobs = []
    for tag, tree in (("before", o.before), ("after", o.after)):
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        jobs += [(tree, u, os.path.join(work, tag, u + ".s")) for u in untouched + edited]
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(lambda j: compile_unit(*j), jobs))
    print("| unit | assembly |\n|---|---|")
    for u in untouched:
        a, b = (open(os.path.join(work, t, u + ".s"), "rb").read() for t in ("before", "after"))
        print("| %s | %s |" % (u, "byte-identical (%d bytes)" % len(a) if a == b else "DIFFERS"))
    print("\n| kernel | " + " | ".join(COLS) + " | instr change |\n|---|" + "---|" * (len(COLS) + 1))
    for u in edited:
        kb, ka = (kernels_of(os.path.join(work, t, u + ".s"), pattern) for t in ("before", "after"))
        for name in kb:
            b, a = kb[name], ka.get(name)
            if a is None:
                print("| %s | missing after |" % name)
                continue
            cells = ["%d" % b[c] if a[c] == b[c] else "%d -> %d" % (b[c], a[c]) for c in COLS]
            print("| `%s` | %s | %+.2f %% |" % (name, " | ".join(cells), 100.0 * (a["instr"] - b["instr"]) / b["instr"]))


if __name__ == "__main__":
    main()
