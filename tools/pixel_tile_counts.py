#!/usr/bin/env python3
"""Before / after counter for the pixel-tile kernels (profiles/pixel_tile/README.md): compiles every kernel unit of two source trees to
gfx950 assembly with each tree's own Makefile flags (make -pn) and prints (markdown)
  * whether the assembly of the units that do NOT include csrc/mcrt_pixels.h is byte-identical, and
  * for every instantiation of k_bmode, k_compound, k_volume, k_label_gather and k_render: registers, scratch, LDS, occupancy (the
    compiler's own kernel info, the figures `make resources` prints), the instruction count and the counts of global loads, global
    stores and ds_bpermute.

  tools/pixel_tile_counts.py BEFORE_TREE AFTER_TREE [WORKDIR]      (a tree: a checkout's root)

-cuid=0 pins the compile-unit id, which otherwise hashes the source's path into a symbol name.  Needs no GPU.  It asserts on nothing."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

UNTOUCHED = ["mcrt_walk", "mcrt_shade", "mcrt_path", "mcrt_march", "mcrt_post", "mcrt_speckle", "mcrt_recon", "mcrt_scene", "mcrt_lbvh"]
EDITED = ["mcrt_display", "mcrt_volume", "mcrt_label", "mcrt_render"]
KERNELS = re.compile(r"mcrt::(k_bmode<|k_compound<|k_volume<|k_label_gather\(|k_render<)")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INFO = {"vgpr": r"; NumVgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)", "lds": r"; LDSByteSize: (\d+)", "occ": r"; Occupancy: (\d+)"}
COLS = ["vgpr", "sgpr", "scratch", "lds", "occ", "instr", "gload", "gstore", "bperm"]


def flags_of(tree):
    """CXXFLAGS and HIPFLAGS as the tree's own Makefile sets them"""
    db = subprocess.run(["make", "-pn", "-C", os.path.join(tree, "mcray-tracing_amd")], capture_output=True, text=True).stdout
    return [w for var in ("CXXFLAGS", "HIPFLAGS") for w in re.search(r"^%s :?= (.*)$" % var, db, re.M).group(1).split()]


def compile_unit(tree, unit, out):
    src = os.path.join(tree, "mcray-tracing_amd", "csrc", unit + ".hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950"] + flags_of(tree) + ["--cuda-device-only", "-S", "-cuid=0", "-o", out, src], capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s does not compile:\n%s" % (src, r.stderr))


def kernels_of(path):
    """{demangled kernel name: counts}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:.*?; Kernel info:\n(.*?)\n\s*\.", text, re.M | re.S):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        if not KERNELS.search(name):
            continue
        ins = [l.split()[0] for l in m.group(2).splitlines() if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
        row = {k: int(re.search(p, m.group(3)).group(1)) for k, p in INFO.items()}
        row.update(instr=len(ins), gload=sum(i.startswith("global_load") for i in ins), gstore=sum(i.startswith("global_store") for i in ins),
                   bperm=sum(i == "ds_bpermute_b32" for i in ins))
        out[re.sub(r"^void mcrt::|\(mcrt::\w+\)$", "", name)] = row
    return out


def main():
    before, after = sys.argv[1], sys.argv[2]
    work = sys.argv[3] if len(sys.argv) > 3 else "build/pixel_tile_counts"
    jobs = []
    for tag, tree in (("before", before), ("after", after)):
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        jobs += [(tree, u, os.path.join(work, tag, u + ".s")) for u in UNTOUCHED + EDITED]
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(lambda j: compile_unit(*j), jobs))
    print("| unit | assembly |\n|---|---|")
    for u in UNTOUCHED:
        a, b = (open(os.path.join(work, t, u + ".s"), "rb").read() for t in ("before", "after"))
        print("| %s | %s |" % (u, "byte-identical (%d bytes)" % len(a) if a == b else "DIFFERS"))
    print("\n| kernel | " + " | ".join(COLS) + " | instr change |\n|---|" + "---|" * (len(COLS) + 1))
    for u in EDITED:
        kb, ka = (kernels_of(os.path.join(work, t, u + ".s")) for t in ("before", "after"))
        for name in kb:
            b, a = kb[name], ka.get(name)
            if a is None:
                print("| %s | missing after |" % name)
                continue
            cells = ["%d" % b[c] if a[c] == b[c] else "%d -> %d" % (b[c], a[c]) for c in COLS]
            print("| `%s` | %s | %+.2f %% |" % (name, " | ".join(cells), 100.0 * (a["instr"] - b["instr"]) / b["instr"]))


if __name__ == "__main__":
    main()
