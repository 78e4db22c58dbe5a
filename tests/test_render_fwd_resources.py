"""CPU: the register budget of the SDF-only skip marcher (the kernel bench.py times), as the gfx950 compiler reports it.

render_fwd_pixgrid<so_row<0, false>, March::SkipFaceSafe> runs at 8 waves / SIMD only with <= 64 VGPRs (allocation granule 8) and <= 80 SGPRs
(a CU admits floor(800 / (ceil(sgpr / 16) * 16 + 16)) blocks of 256 threads), and without scratch.  The rare canonical
cell selection near voxel faces re-derives the ray and the mapping inside its branch instead of keeping them live across
the march loop; this test keeps a later change from quietly bringing them back."""
import shutil

import pytest

from kernel_report import HIPCC, Row, kernels_of

SKIP_FACE_SAFE = "((anonymous namespace)::March)4"     # enum class March of render_fwd.hip, as c++filt prints it


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
def test_skip_marcher_fits_eight_waves_per_simd():
    hits = [k for k in kernels_of("render_fwd.hip", "render_fwd_pixgrid", lambda r: r == Row(0, False, 0, False))
            if k.rest == SKIP_FACE_SAFE]
    assert len(hits) == 1, hits
    r = hits[0].res
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r
    assert r["TotalSGPRs"] <= 80, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 8, r
