#!/usr/bin/env python3
"""Do two versions of a kernel file compile to the same gfx950 code?  The acceptance check of a refactor of csrc/*.hip.

usage: scripts/kernel_isa_diff.py OLD NEW FILE.hip [FILE.hip ...]
OLD / NEW: a source tree (a directory), or a git revision of this repository (unpacked into a temp dir with git archive).
FILE: a name under selfocc_amd/csrc.

Each file is compiled device-only with the flags of csrc/build.sh and disassembled.  A function is its instruction stream
together with its row of the compiler's resource table, so a kernel may change its (mangled) name but nothing else.  While
both trees emit their functions in the same order they are compared position by position; when the order differs (a merged
launcher instantiates its kernels in another order) every function is PAIRED BY CONTENT, position ignored, and what is left
over on either side is reported: each leftover of OLD next to the nearest leftover of NEW, with their diff.  Names are
printed demangled.  Exit status 1 if any function is left unpaired."""
import collections
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
            if insn and insn != "...":                      # "...": the padding objdump elides after a function
                out[-1][1].append(insn)
    return out


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def pair(old, new):
    """(emission order kept?, [(old function, new function or None)] of what differs, [new functions without a partner])"""
    if len(old) == len(new):
        diff = [(o, n) for o, n in zip(old, new) if o[1:] != n[1:]]
        if not diff:
            return True, [], []
    key = lambda f: (tuple(f[1]), tuple(sorted(f[2].items())))
    pool = collections.defaultdict(list)
    for f in new:
        pool[key(f)].append(f)
    left_old = [f for f in old if not (pool[key(f)] and pool[key(f)].pop())]
    left_new = [f for fs in pool.values() for f in fs]
    pairs = []
    for o in left_old:   # the nearest leftover of the other side: same resources first, then the closest length
        n = min(left_new, key=lambda f: (f[2] != o[2], abs(len(f[1]) - len(o[1]))), default=None)
        if n is not None:
            left_new.remove(n)
        pairs.append((o, n))
    return False, pairs, left_new


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
            jobs = {(f, i): pool.submit(kernels, t, f, os.path.join(tmp, "%d_%s.co" % (i, f)))
                    for f in argv[2:] for i, t in enumerate(trees)}
        for f in argv[2:]:
            old, new = (jobs[(f, i)].result() for i in range(2))
            same_order, pairs, extra = pair(old, new)
            names = demangle([x[0] for p in pairs for x in p if x] + [x[0] for x in extra])
            for o, n in pairs:
                if n is None:
                    print("ONLY IN OLD %s: %s" % (f, names[o[0]]))
                    continue
                print("DIFFERS %s: %s -> %s" % (f, names[o[0]], names[n[0]]))
                print("  instructions: %d -> %d" % (len(o[1]), len(n[1])))
                if o[2] != n[2]:
                    print("  resources: %s -> %s" % (o[2], n[2]))
                for line in list(difflib.unified_diff(o[1], n[1], "old", "new", n=2, lineterm=""))[:60]:
                    print("  " + line)
            for n in extra:
                print("ONLY IN NEW %s: %s" % (f, names[n[0]]))
            bad = len(pairs) + len(extra)
            print("%s: %d / %d functions, emission order %s, %d unpaired" % (f, len(old), len(new),
                                                                           "unchanged" if same_order else "changed", bad))
            differing += bad
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
