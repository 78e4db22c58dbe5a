"""CPU: the register budget of the SDF-only skip marcher (the kernel bench.py times), as the gfx950 compiler reports it.

render_fwd_pixgrid<0, false, March::SkipFaceSafe> runs at 8 waves / SIMD only with <= 64 VGPRs (allocation granule 8) and <= 80 SGPRs
(a CU admits floor(800 / (ceil(sgpr / 16) * 16 + 16)) blocks of 256 threads), and without scratch.  The rare canonical
cell selection near voxel faces re-derives the ray and the mapping inside its branch instead of keeping them live across
the march loop; this test keeps a later change from quietly bringing them back."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags of selfocc_amd/csrc/build.sh
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
         "-fno-vectorize", "--cuda-device-only", "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]


def _resources(src):
    out = subprocess.run([HIPCC, *FLAGS, src], check=True, capture_output=True, text=True).stderr
    table, name = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            table[name] = {}
            continue
        m = re.search(r"remark: +(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            table[name][m.group(1).split()[0]] = int(m.group(2))
    return table


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
def test_skip_marcher_fits_eight_waves_per_simd():
    table = _resources(os.path.join(ROOT, "selfocc_amd", "csrc", "render_fwd.hip"))
    # _ZN12_GLOBAL__N_118render_fwd_pixgridILi0ELb0ELNS_5MarchE4EEEv14so_render_argsii = render_fwd_pixgrid<0, false, March::SkipFaceSafe>
    hits = {k: v for k, v in table.items() if "render_fwd_pixgridILi0ELb0ELNS_5MarchE4E" in k}
    assert len(hits) == 1, sorted(table)
    r = next(iter(hits.values()))
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r
    assert r["TotalSGPRs"] <= 80, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 8, r
