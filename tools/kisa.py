#!/usr/bin/env python3
"""Instruction multiset of every kernel of one csrc source, for comparing two trees with diff:
tools/kisa.py powerflow.hip [f64 | vmem | all]        (a path with a directory names a source of another tree)
One line per (kernel, mnemonic): f64 the v_*_f64 only, vmem (default) the vector-ALU, LDS and global-memory ones, all every one.
The encoding suffixes _e32 / _e64 are dropped; a call (s_swappc_b64) is listed in every mode: nothing may stay un-inlined."""
import collections, os, re, subprocess, sys, tempfile
src = sys.argv[1]
csrc = os.path.dirname(src) or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "poweflownet_amd", "csrc")
mode = sys.argv[2] if len(sys.argv) > 2 else "vmem"
keep = {"f64": r"v_\w+_f64", "vmem": r"(v_|ds_|global_|flat_|buffer_|scratch_)\w+", "all": r"\w+"}[mode] + r"|s_swappc_b64"
with tempfile.TemporaryDirectory() as tmp:
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-save-temps=obj", "-c", os.path.basename(src),
                    "-o", os.path.join(tmp, "k.o")], cwd=csrc, check=True, capture_output=True)
    asm = open(os.path.join(tmp, os.path.basename(src)[:-4] + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
cur, counts = None, collections.defaultdict(collections.Counter)
for line in asm.splitlines():
    m = re.match(r"(_Z\w+):", line)
    if m: cur = m.group(1); continue
    if line.startswith(".Lfunc_end"): cur = None; continue
    m = re.match(r"\t([a-z]\w+)", line)
    if m and cur and re.fullmatch(keep, m.group(1)): counts[cur][re.sub(r"_e(32|64)$", "", m.group(1))] += 1
for name, c in counts.items():
    short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
    for mnem in sorted(c): print(f"{short}\t{mnem}\t{c[mnem]}")
