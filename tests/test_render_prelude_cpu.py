"""CPU: what the skip marcher and the brick pass no longer compute per wave or per cell, as the gfx950 compiler emits them.

The launch's constants (per axis size0 / range0, the skip unit's square root and division) come from the host in a kernel
argument (csrc/render_fwd.hip, so_launch_consts), and the pixel-grid skip marcher reads tile and camera from blockIdx.
render_fwd.hip is compiled to assembly with the flags of csrc/build.sh, as tests/kernel_report.py invokes the compiler, and
ordinary arithmetic instructions are counted inside the body of one kernel at a time:

  render_fwd_pixgrid<so_row<0, false>, March::SkipFaceSafe> (the kernel bench.py times)
      v_rcp_iflag_f32   0      (before: 2, the two integer divisions of the linear tile index)
      v_div_scale    <= 74     (before: 82; two per IEEE division: the three axis divisions and the skip unit's are gone)
      v_sqrt_f32     <= 1      (before: 2; the ray's direction norm stays)
  sdf_brickify_kernel
      v_div_scale    <= 6      (before: 14; three divisions per cell stay: 17.5 / inv_s, slack / G, / unit)
      v_sqrt_f32     <= 1      (before: 2; the gradient bound's stays)
"""
import functools
import re
import shutil
import subprocess

import pytest

from kernel_report import FLAGS, HIPCC, ROOT

pytestmark = pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")

SKIP_FACE_SAFE = "((anonymous namespace)::March)4"     # enum class March of render_fwd.hip, as c++filt prints it


@functools.lru_cache(maxsize=None)
def bodies():
    """demangled kernel name -> the instructions of its body (mnemonic first), from the assembly of render_fwd.hip"""
    flags = [f for f in FLAGS if not f.startswith("-Rpass")]
    flags[flags.index("-c")] = "-S"
    flags[flags.index("-o") + 1] = "-"
    asm = subprocess.run([HIPCC, *flags, f"{ROOT}/selfocc_amd/csrc/render_fwd.hip"], check=True, capture_output=True,
                         text=True).stdout
    out, sym, cur = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            sym, cur = m.group(1), []
        elif cur is not None and line.startswith(".Lfunc_end"):
            out[sym], cur = cur, None
        elif cur is not None:
            text = line.split(";")[0].strip()
            if text and not text.startswith(".") and not text.endswith(":"):
                cur.append(text)
    names = subprocess.run(["c++filt"], input="\n".join(out), check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(names) == len(out)
    return dict(zip(names, out.values()))


def body_of(*parts):
    hits = [b for n, b in bodies().items() if all(p in n for p in parts)]
    assert len(hits) == 1, (parts, [n for n in bodies() if parts[0] in n])
    assert len(hits[0]) > 100, (parts, len(hits[0]))      # a kernel's body, not a stub
    return hits[0]


def count(body, mnemonic):
    return sum(1 for text in body if text.split()[0].startswith(mnemonic))


def test_skip_marcher_prelude():
    body = body_of("render_fwd_pixgrid<so_row<0, false, 0, false>", SKIP_FACE_SAFE)
    got = {m: count(body, m) for m in ("v_rcp_iflag_f32", "v_div_scale", "v_sqrt_f32")}
    print(f"[prelude] SkipFaceSafe pixel-grid kernel: {len(body)} instructions, {got}")
    assert got["v_rcp_iflag_f32"] == 0, got
    assert got["v_div_scale"] <= 74, got
    assert got["v_sqrt_f32"] <= 1, got


def test_brick_pass_constants():
    body = body_of("sdf_brickify_kernel(")
    got = {m: count(body, m) for m in ("v_div_scale", "v_sqrt_f32")}
    print(f"[prelude] sdf_brickify_kernel: {len(body)} instructions, {got}")
    assert got["v_div_scale"] <= 6, got
    assert got["v_sqrt_f32"] <= 1, got
