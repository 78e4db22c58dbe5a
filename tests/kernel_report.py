"""What the gfx950 compiler reports for the kernels of one file of selfocc_amd/csrc (a helper of the CPU tests, not a test).

The file is compiled device-only with the flags of csrc/build.sh; the rows of -Rpass-analysis=kernel-resource-usage are parsed
and the names demangled with c++filt.  The render kernels are templates over their feature row (csrc/render_row.h), so a test
picks them by what they are: the template's base name and the row so_row<NF, BF16, NB, MASKED> in the demangled name."""
import collections
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags of selfocc_amd/csrc/build.sh
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
         "-fno-vectorize", "--cuda-device-only", "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
ROWS = r"TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]"

Row = collections.namedtuple("Row", "nf bf16 nb masked")
# name: demangled; base: the template's name; row: its so_row argument (None without one); rest: the template arguments after
# the row, as text; res: {"VGPRs": .., "AGPRs": .., "TotalSGPRs": .., "ScratchSize": .., "Occupancy": .., "LDS": ..}
Kernel = collections.namedtuple("Kernel", "name base row rest res")


@functools.lru_cache(maxsize=None)
def report(src):
    """[Kernel] of selfocc_amd/csrc/<src>, in emission order"""
    path = os.path.join(ROOT, "selfocc_amd", "csrc", src)
    out = subprocess.run([HIPCC, *FLAGS, path], check=True, capture_output=True, text=True).stderr
    table, sym = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            sym = m.group(1)
            table[sym] = {}
            continue
        m = re.search(r"remark: +(%s): (\d+)" % ROWS, line)
        if m and sym:
            table[sym][m.group(1).split()[0]] = int(m.group(2))
    names = subprocess.run(["c++filt"], input="\n".join(table), check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(names) == len(table)
    kernels = []
    for name, res in zip(names, table.values()):
        m = re.search(r"(\w+)<so_row<(\d+), (true|false), (\d+), (true|false)>(?:, (.*))?>\(", name)
        if m:
            row = Row(int(m.group(2)), m.group(3) == "true", int(m.group(4)), m.group(5) == "true")
            kernels.append(Kernel(name, m.group(1), row, m.group(6) or "", res))
        else:
            kernels.append(Kernel(name, re.search(r"(\w+)(?:<.*>)?\(", name).group(1), None, "", res))
    return kernels


def kernels_of(src, base, row=lambda r: True):
    """the instances of template `base` whose row satisfies `row`"""
    return [k for k in report(src) if k.base == base and k.row is not None and row(k.row)]
