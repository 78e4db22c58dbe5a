"""CPU: the register budget of the SDF-only skip marcher without face-safe cell selection, as the gfx950 compiler reports it.

render_fwd_pixgrid<so_row<0, false>, March::Skip> is the instance `face_safe=False` launches.  It shares so_march_fast_ahead
with March::SkipFaceSafe (tests/test_render_fwd_resources.py) and has the same budget for 8 waves / SIMD: <= 64 VGPRs,
<= 80 SGPRs (a CU admits floor(800 / (ceil(sgpr / 16) * 16 + 16)) blocks of 256 threads), no scratch.  The march keeps two
located steps and, in three phases, more than one copy of the step's code; a loop structure that keeps what one phase needs
live across the others costs this instance its 8th wave as quietly as the face-safe one."""
import shutil

import pytest

from kernel_report import HIPCC, Row, kernels_of

SKIP = "((anonymous namespace)::March)3"     # enum class March of render_fwd.hip, as c++filt prints it


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
def test_skip_marcher_without_face_safe_fits_eight_waves_per_simd():
    hits = [k for k in kernels_of("render_fwd.hip", "render_fwd_pixgrid", lambda r: r == Row(0, False, 0, False))
            if k.rest == SKIP]
    assert len(hits) == 1, hits
    r = hits[0].res
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r
    assert r["TotalSGPRs"] <= 80, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 8, r
