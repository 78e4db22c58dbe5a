"""CPU: the 'linear_upscale' mapping (NonLinearMapping, mappings.py:199-288) on the C ABI — the so_mapping constants
``to_abi()`` fills, the struct layout against the ctypes mirror, and the parameter validation on both sides of the boundary
(host and ``so_validate_mapping``, which runs before anything touches a GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from selfocc_amd import abi
from selfocc_amd.mapping import GridMeterMapping

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the golden 'upscale' config (tests/golden/geometry.npz) and the commented nuScenes alternative
# (config/nuscenes/nuscenes_depth.py: bev_inner = 160, bev_outer = 1, range 80 / 1, z 20 / 10 over [-4, 4, 12])
UPSCALE = {
    'golden': dict(nonlinear_mode='linear_upscale', h_size=[128, 32], h_range=[51.2, 28.8], w_size=[128, 32],
                   w_range=[51.2, 28.8], d_size=[20, 10], d_range=[-4.0, 4.0, 12.0]),
    'nuscenes_alt': dict(nonlinear_mode='linear_upscale', h_size=[160, 1], h_range=[80, 1], w_size=[160, 1],
                         w_range=[80, 1], d_size=[20, 10], d_range=[-4, 4, 12]),
}


def _reference_constants(inner, outer, r_inner, r_outer):
    """the reference's own Python (double) expressions, mappings.py:222-226 and :260-262"""
    unit = r_inner * 1.0 / inner
    inc = (r_outer - outer * unit) * 2.0 / outer / (outer + 1)
    c = 1. / 2 + unit / inc
    return unit, inc, c, c ** 2


def _f32(x):
    return float(np.float32(x))


@pytest.mark.parametrize("name", list(UPSCALE))
def test_to_abi_fills_the_upscale_kind_and_float32_of_the_reference_constants(name):
    kw = UPSCALE[name]
    m = GridMeterMapping(**kw).to_abi()
    assert m.kind == abi.MAP_UPSCALE == 1
    inner, outer = kw['h_size']
    r_in, r_out = kw['h_range']
    z0, z1, z2 = kw['d_range']
    for u in (m.uh, m.uw):
        assert (u.unit, u.inc, u.c, u.c2) == tuple(_f32(v) for v in _reference_constants(inner, outer, r_in, r_out))
    zi, zo = kw['d_size']
    assert (m.ud.unit, m.ud.inc, m.ud.c, m.ud.c2) == tuple(_f32(v) for v in _reference_constants(zi, zo, z1 - z0, z2 - z1))
    for ax in (m.h, m.w):
        assert (ax.size0, ax.size1, ax.range0, ax.range1) == (inner, outer, _f32(r_in), _f32(r_out))
        assert (ax.off0, ax.off1, ax.start, ax.tot_len) == (inner, outer, 0.0, 1 + 2 * (inner + outer))
    assert (m.d.size0, m.d.size1, m.d.range0, m.d.range1) == (zi, zo, _f32(z1 - z0), _f32(z2 - z1))
    assert (m.d.off0, m.d.off1, m.d.start, m.d.tot_len) == (0.0, 0.0, _f32(z0), 1 + zi + zo)


def test_linear_to_abi_keeps_the_zero_kind():
    m = GridMeterMapping(nonlinear_mode='linear', h_size=[128, 0], h_range=[40.0, 0], w_size=[128, 0], w_range=[40.0, 0],
                         d_size=[24, 0], d_range=[-1.0, 5.4, 5.4]).to_abi()
    assert m.kind == abi.MAP_LINEAR == 0
    assert abi.SoMapping().kind == abi.MAP_LINEAR          # a hand-filled (zero-initialised) mapping is linear


def test_upscale_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of the mapping-kind fields (and of the argument structs that embed so_mapping) against ctypes"""
    fields = [("so_upscale_axis", f, abi.SoUpscaleAxis) for f in ("unit", "inc", "c", "c2")] + \
             [("so_mapping", f, abi.SoMapping) for f in ("h", "w", "d", "kind", "_pad", "uh", "uw", "ud")] + \
             [("so_render_args", "sdf_vol", abi.SoRenderArgs), ("so_render_args", "inv_s_dev", abi.SoRenderArgs),
              ("so_render_bwd_args", "g_depth", abi.SoRenderBwdArgs), ("so_query_args", "sdf_vol", abi.SoQueryArgs),
              ("so_query_args", "sem_argmax", abi.SoQueryArgs)]
    body = "\n".join(f'printf("%zu %zu\\n", sizeof({s}), offsetof({s}, {f}));' for s, f, _ in fields)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/selfocc_hip.h"\n'
                   f'int main(void) {{ {body} return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    for (s, f, cls), line in zip(fields, lines):
        size, off = map(int, line.split())
        assert C.sizeof(cls) == size, (s, C.sizeof(cls), size)
        assert getattr(cls, f).offset == off, (s, f, getattr(cls, f).offset, off)
    # the kind fields add 64 bytes: the argument-struct fields after so_mapping keep their offsets mod 64
    assert C.sizeof(abi.SoMapping) == 3 * C.sizeof(abi.SoAxis) + 64


@pytest.mark.parametrize("kw,msg", [
    (dict(h_size=[128, 0], w_size=[128, 0]), "linear_upscale axis 0: outer cells must be >= 1 (got 0)"),
    (dict(d_size=[20, 0]), "linear_upscale axis 2: outer cells must be >= 1 (got 0)"),
])
def test_host_rejects_zero_outer_cells(kw, msg):
    with pytest.raises(ValueError) as e:
        GridMeterMapping(**{**UPSCALE['golden'], **kw})
    assert str(e.value) == msg


@pytest.mark.parametrize("kw,axis", [
    (dict(h_range=[51.2, 5.0], w_range=[51.2, 5.0]), 0),     # 32 outer cells of >= 0.4 m cannot cover 5 m
    (dict(d_range=[-4.0, 4.0, 6.0]), 2),                     # 10 outer cells of >= 0.4 m cannot cover 2 m
])
def test_host_and_c_boundary_reject_a_non_positive_increase_unit_with_one_message(kw, axis):
    m = GridMeterMapping(**{**UPSCALE['golden'], **kw})
    with pytest.raises(ValueError) as e:
        m.to_abi()
    host_msg = str(e.value)
    assert host_msg.startswith(f"linear_upscale axis {axis}: increase unit must be > 0 (got ")
    # the same constants, past the host check, through the C boundary
    inc = m.mapping.increase_unit if axis < 2 else m.mapping.z_increase_unit
    good = GridMeterMapping(**UPSCALE['golden']).to_abi()
    for u in ((good.uh, good.uw) if axis < 2 else (good.ud,)):
        u.inc = inc
    from selfocc_amd._lib import lib
    l = lib()
    assert l.selfocc_meter2grid(good, None, 1, 0, None, None) == -1
    assert l.selfocc_last_error().decode() == host_msg


def test_c_boundary_rejects_unknown_kind_and_zero_outer_cells():
    from selfocc_amd._lib import lib
    l = lib()
    m = GridMeterMapping(**UPSCALE['golden']).to_abi()
    m.kind = 7
    assert l.selfocc_meter2grid(m, None, 0, 0, None, None) == -1
    assert "unknown kind 7" in l.selfocc_last_error().decode()
    m = GridMeterMapping(**UPSCALE['golden']).to_abi()
    m.d.size1 = 0.0
    assert l.selfocc_meter2grid(m, None, 0, 0, None, None) == -1
    assert l.selfocc_last_error().decode() == "linear_upscale axis 2: outer cells must be >= 1 (got 0)"
    # a valid mapping with nothing to do returns before any launch
    assert l.selfocc_meter2grid(GridMeterMapping(**UPSCALE['golden']).to_abi(), None, 0, 0, None, None) == 0
