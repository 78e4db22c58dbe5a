#!/usr/bin/env python3
"""Do two versions of a kernel file compile to the same gfx950 code?  The acceptance check of a refactor of csrc/*.hip.

usage: scripts/kernel_isa_diff.py OLD NEW FILE.hip [FILE.hip ...]
OLD / NEW: a source tree (a directory), or a git revision of this repository (unpacked into a temp dir with git archive).
FILE: a name under selfocc_amd/csrc.

Each file is compiled device-only with the flags of csrc/build.sh and disassembled.  The functions are compared in EMISSION
ORDER, instruction stream by instruction stream, together with their rows of the compiler's resource table, so a kernel may
change its (mangled) name but nothing else.  Prints the counts and every function that differs; exit status 1 if any does."""
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
# the flags of selfocc_amd/csrc/build.sh
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
         "-fno-vectorize", "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-Rpass-analysis=kernel-resource-usage"]
ROWS = r"TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]"


def kernels(tree, name, obj):
    """[(symbol, [instruction, ...], {resource: value})] of one file, in emission order"""
    cc = subprocess.run([HIPCC, *FLAGS, os.path.join(tree, "selfocc_amd", "csrc", name), "-o", obj], capture_output=True, text=True)
    if cc.returncode:
        sys.exit("%s of %s does not compile:\n%s" % (name, tree, "\n".join(l for l in cc.stderr.splitlines() if "remark:" not in l)))
    err = cc.stderr
    res, sym = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            sym = m.group(1)
            res[sym] = {}
        m = re.search(r"remark: +(%s): (\d+)" % ROWS, line)
        if m and sym:
            res[sym][m.group(1)] = int(m.group(2))
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", obj], check=True, capture_output=True,
                         text=True).stdout
    out = []
    for line in dis.splitlines():
        m = re.match(r"<(\S+)>:$", line)
        if m:
            out.append((m.group(1), [], res.get(m.group(1), {})))
        elif out and line.startswith(("\t", " ")):
            insn = " ".join(line.split("//")[0].split())    # drop the "// address: encoding <symbol+off>" comment
            if insn:
                out[-1][1].append(insn)
    return out


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    differing = 0
    with tempfile.TemporaryDirectory() as tmp:
        trees = []
        for i, t in enumerate(argv[:2]):
            if not os.path.isdir(t):   # a git revision
                d = os.path.join(tmp, "tree%d" % i)
                os.mkdir(d)
                tar = subprocess.run(["git", "-C", ROOT, "archive", t, "selfocc_amd/csrc", "include"], check=True, capture_output=True)
                subprocess.run(["tar", "-x", "-C", d], input=tar.stdout, check=True)
                t = d
            trees.append(os.path.abspath(t))
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            jobs = {(f, t): pool.submit(kernels, t, f, os.path.join(tmp, "%d_%s.co" % (i, f)))
                    for f in argv[2:] for i, t in enumerate(trees)}
        for f in argv[2:]:
            old, new = (jobs[(f, t)].result() for t in trees)
            bad = abs(len(old) - len(new))
            for (so, io, ro), (sn, inew, rn) in zip(old, new):
                if io == inew and ro == rn:
                    continue
                bad += 1
                print("DIFFERS %s: %s -> %s" % (f, so, sn))
                if ro != rn:
                    print("  resources: %s -> %s" % (ro, rn))
                for line in list(difflib.unified_diff(io, inew, "old", "new", n=2, lineterm=""))[:60]:
                    print("  " + line)
            print("%s: %d / %d functions, %d differing" % (f, len(old), len(new), bad))
            differing += bad
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
