"""CPU: the rendered normal (selfocc_render_normal) — the symbol, the unchanged ABI version, the struct
layout against the header, the host-side refusals, and the CPU definition `normal_vis_reference`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from selfocc_amd import abi
import median_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_point_without_a_version_bump():
    from selfocc_amd._lib import lib
    l = lib()
    assert abi.ABI_VERSION == 35 == l.selfocc_abi_version()       # only a new entry point: no version bump
    assert 'selfocc_render_normal' in abi.SYMBOLS and hasattr(l, 'selfocc_render_normal')
    import selfocc_amd
    from selfocc_amd import render
    assert selfocc_amd.render_normal_vis is render.render_normal_vis
    assert selfocc_amd.normal_vis_reference is render.normal_vis_reference


def test_normal_args_layout_matches_the_header(tmp_path):
    fields = ('fwd', 'normal_vis')
    assert [f for f, _ in abi.SoRenderNormalArgs._fields_] == list(fields)
    body = "\n".join(f'printf("%zu %zu\\n", sizeof(so_render_normal_args), offsetof(so_render_normal_args, {f}));' for f in fields)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/selfocc_hip.h"\n'
                   f'int main(void) {{ {body} printf("%zu\\n", sizeof(so_render_args)); return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    for f, line in zip(fields, lines):
        size, off = map(int, line.split())
        assert size == C.sizeof(abi.SoRenderNormalArgs) and off == getattr(abi.SoRenderNormalArgs, f).offset, f
    assert int(lines[2]) == C.sizeof(abi.SoRenderArgs) == abi.SoRenderNormalArgs.normal_vis.offset   # so_render_args untouched


def _args(out=True, **kw):
    """a launch that passes every check; with n_rays = 0 it returns before anything touches a device"""
    m = abi.SoRenderNormalArgs()
    a = m.fwd
    for ax, n in ((a.map.h, 17), (a.map.w, 17), (a.map.d, 9)):
        ax.tot_len, ax.size0, ax.range0 = n, float(n - 1), 12.8
    m.keep = C.create_string_buffer(64)          # never dereferenced
    a.sdf_vol = a.origins = a.dirs = C.addressof(m.keep)
    a.n_samples, a.n_rays, a.ray_mode = 32, 0, abi.RAYS_EXPLICIT
    if out:
        m.normal_vis = C.addressof(m.keep)
    for k, v in kw.items():
        setattr(a, k, v)
    return m


def test_host_refusals_name_the_field():
    """every refusal is host logic, before any HIP call: rc < 0 and the field's name in selfocc_last_error()"""
    from selfocc_amd._lib import lib
    l = lib()
    ok = [_args(), _args(n_samples=1),
          # the feature fields, the flags and the outputs of the embedded struct are ignored, whatever they hold
          _args(n_rgb=7, n_sem=99, feat_stride=5, feat_dtype=9, sh_deg=11, sh_act=5, bkgd_mode=abi.BKGD_PER_RAY, flags=-1)]
    for m in ok:
        assert l.selfocc_render_normal(m, None) == 0, l.selfocc_last_error()        # n_rays = 0: success, no launch
    bad = [(_args(out=False), b"normal_vis"), (_args(n_samples=0), b"n_samples"), (_args(n_samples=-3), b"n_samples"),
           (_args(n_rays=-1), b"n_rays"), (_args(sdf_vol=None), b"sdf_vol"), (_args(sample_pos=2), b"sample_pos"),
           (_args(jitter_mode=abi.JITTER_SINGLE), b"t_rand"), (_args(ray_mode=5), b"ray_mode")]
    for m, word in bad:
        assert l.selfocc_render_normal(m, None) < 0, word
        err = l.selfocc_last_error()
        assert word in err, (word, err)
    # a NULL output is refused even when there are rays to march (before the launch, so the dummy pointers are never read)
    assert l.selfocc_render_normal(_args(out=False, n_rays=5), None) < 0 and b"normal_vis" in l.selfocc_last_error()
    assert l.selfocc_render_normal(None, None) < 0 and b"args" in l.selfocc_last_error()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def test_reference_on_a_hand_made_case():
    """2 rays x 3 samples, worked by hand in float32.
    Ray 0: w = (0.5, 0.25, 0);  g = (3, 0, 4) -> r = 5, n = (fl(0.6), 0, fl(0.8));  g = 0 -> d = 1e-12 (the clamp), n = 0, so the
      weight 0.25 adds nothing;  g = (0, -2, 0) -> n = (0, -1, 0) under a ZERO weight adds -0.
      N = (0.5 fl(0.6), 0, 0.5 fl(0.8)) = (0x3E99999A, 0, 0x3ECCCCCD).  x: 1 + 0x3E99999A drops the bits '10', a tie, to even:
      0x3FA66666, halved 0x3F266666.  z: 1 + 0x3ECCCCCD drops '01', down: 0x3FB33333, halved 0x3F333333.  y: exactly 0.5.
    Ray 1: w = (0.3, 0.2, 0.1);  g = (1, 2, 2) -> r = 3, n = (fl(1/3), fl(2/3), fl(2/3));  g = 0 -> n = 0;  g = (0, 0, -0.5) ->
      n = (0, 0, -1).  N = (fl(0.3f fl(1/3)), fl(0.3f fl(2/3)), fl(0.3f fl(2/3)) - 0.1f)."""
    from selfocc_amd.render import normal_vis_reference
    w = torch.tensor([[0.5, 0.25, 0.0], [0.3, 0.2, 0.1]])
    g = torch.tensor([[[3.0, 0.0, 4.0], [0.0, 0.0, 0.0], [0.0, -2.0, 0.0]], [[1.0, 2.0, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, -0.5]]])
    want = np.array([[0x3F266666, 0x3F000000, 0x3F333333], [0x3F0CCCCD, 0x3F19999A, 0x3F0CCCCD]], dtype=np.uint32)
    got = normal_vis_reference(w, g)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.shape == (2, 3)
    assert np.array_equal(_bits(got.numpy()), want), [[hex(v) for v in row] for row in _bits(got.numpy())]
    # arrays in, array out
    arr = normal_vis_reference(w.numpy(), g.numpy())
    assert isinstance(arr, np.ndarray) and np.array_equal(_bits(arr), want)


def _loop_reference(w, g):
    """the contract, one ray, one sample and one float32 operation at a time.  The square root and the divisions are taken in
    double and rounded once more: for these two operations that is the correctly rounded float32 result (53 >= 2 * 24 + 2)"""
    f, f64 = np.float32, np.float64
    out = np.zeros((w.shape[0], 3), dtype=f)
    for r in range(w.shape[0]):
        N = [f(0.0)] * 3
        for i in range(w.shape[1]):
            gx, gy, gz = g[r, i]
            d = max(f(np.sqrt(f64(f(f(gx * gx) + f(gy * gy)) + f(gz * gz)))), f(1e-12))
            for k in range(3):
                N[k] = f(N[k] + f(w[r, i] * f(f64(g[r, i, k]) / f64(d))))
        out[r] = [f(f(n + f(1.0)) / f(2.0)) for n in N]
    return out


def test_reference_equals_a_plain_loop_in_sample_order():
    """random rows, with zero gradients and zero weights sprinkled in; S = 70 so that the order of the sum matters: a
    pairwise or double-precision sum gives other bits on some rows"""
    from selfocc_amd.render import normal_vis_reference
    rng = np.random.RandomState(2)
    n, S = 40, 70
    w = (rng.uniform(0, 1, (n, S)) ** 6).astype(np.float32)
    g = rng.normal(0, 1, (n, S, 3)).astype(np.float32)
    w[rng.uniform(size=(n, S)) < 0.1] = 0.0
    g[rng.uniform(size=(n, S)) < 0.1] = 0.0
    want = _loop_reference(w, g)
    got = normal_vis_reference(torch.from_numpy(w), torch.from_numpy(g))
    assert np.array_equal(_bits(got.numpy()), _bits(want))
    nrm = g / np.maximum(np.linalg.norm(g.astype(np.float64), axis=-1, keepdims=True), 1e-12)
    other = (((w[..., None].astype(np.float64) * nrm).sum(1) + 1.0) / 2.0).astype(np.float32)
    assert not np.array_equal(_bits(other), _bits(want)) and np.abs(other - want).max() < 1e-5   # the order is part of the definition


def test_render_normal_vis_needs_device_tensors():
    from selfocc_amd.render import render_normal_vis
    vol, aabb = mc.make_volume('linear')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_normal_vis(vol, mc.make_explicit_rays('linear'), mc.make_cfg(aabb))
