"""CPU: the register budget of the SDF-only skip marcher launched on explicit rays, as the gfx950 compiler reports it.

render_fwd_explicit<so_row<0, false>, March::Skip / March::SkipFaceSafe> share so_march_fast_ahead with the pixel-grid
instances (tests/test_render_fwd_resources.py, test_render_fwd_resources_skip.py) and have the same budget for 8 waves / SIMD:
<= 64 VGPRs, <= 80 SGPRs, no scratch.  The face-safe instance sits at 64 VGPRs exactly: a value of a rare block that the
compiler hoists in front of the loops (the |t_mid| bound of the spent-exit test did) costs it its 8th wave while the
pixel-grid instances still fit."""
import shutil

import pytest

from kernel_report import HIPCC, Row, kernels_of

MARCHES = {"skip": "((anonymous namespace)::March)3", "skip_face_safe": "((anonymous namespace)::March)4"}


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
@pytest.mark.parametrize("march", sorted(MARCHES))
def test_explicit_skip_marcher_fits_eight_waves_per_simd(march):
    hits = [k for k in kernels_of("render_fwd.hip", "render_fwd_explicit", lambda r: r == Row(0, False, 0, False))
            if k.rest == MARCHES[march]]
    assert len(hits) == 1, hits
    r = hits[0].res
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r
    assert r["TotalSGPRs"] <= 80, r
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] == 8, r
