"""CPU: the median depth (selfocc_render_median) — struct layout against the header, the unchanged ABI
version, the host-side refusals, the CPU definition `median_depth_reference`, and the head's new keyword."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import torch

from oracle import torch_port as tp
from selfocc_amd import abi, synthetic as sy
import median_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_median_args_layout_matches_the_header(tmp_path):
    fields = ('fwd', 'median_depth', 'median_index')
    assert [f for f, _ in abi.SoRenderMedianArgs._fields_] == list(fields)
    body = "\n".join(f'printf("%zu %zu\\n", sizeof(so_render_median_args), offsetof(so_render_median_args, {f}));' for f in fields)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/selfocc_hip.h"\n'
                   f'int main(void) {{ {body} printf("%zu\\n", sizeof(so_render_args)); return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    for f, line in zip(fields, lines):
        size, off = map(int, line.split())
        assert size == C.sizeof(abi.SoRenderMedianArgs) and off == getattr(abi.SoRenderMedianArgs, f).offset, f
    assert int(lines[3]) == C.sizeof(abi.SoRenderArgs) == abi.SoRenderMedianArgs.median_depth.offset   # so_render_args untouched


def test_new_entry_point_without_a_version_bump():
    from selfocc_amd._lib import lib
    l = lib()
    assert abi.ABI_VERSION == 35 == l.selfocc_abi_version()       # only a new entry point: no version bump
    assert 'selfocc_render_median' in abi.SYMBOLS and hasattr(l, 'selfocc_render_median')
    import selfocc_amd
    from selfocc_amd import render
    assert selfocc_amd.render_median_depth is render.render_median_depth
    assert selfocc_amd.median_depth_reference is render.median_depth_reference


def _args(depth=True, index=True, **kw):
    """a launch that passes every check; with n_rays = 0 it returns before anything touches a device"""
    m = abi.SoRenderMedianArgs()
    a = m.fwd
    for ax, n in ((a.map.h, 17), (a.map.w, 17), (a.map.d, 9)):
        ax.tot_len, ax.size0, ax.range0 = n, float(n - 1), 12.8
    m.keep = C.create_string_buffer(64)          # never dereferenced
    a.sdf_vol = a.origins = a.dirs = C.addressof(m.keep)
    a.n_samples, a.n_rays, a.ray_mode = 32, 0, abi.RAYS_EXPLICIT
    if depth:
        m.median_depth = C.addressof(m.keep)
    if index:
        m.median_index = C.addressof(m.keep)
    for k, v in kw.items():
        setattr(a, k, v)
    return m


def test_host_refusals_name_the_field():
    """every refusal is host logic, before any HIP call: rc < 0 and the field's name in selfocc_last_error()"""
    from selfocc_amd._lib import lib
    l = lib()
    ok = [_args(), _args(index=False), _args(depth=False), _args(n_samples=1),
          # the feature fields, the flags and the outputs of the embedded struct are ignored, whatever they hold
          _args(n_rgb=7, n_sem=99, feat_stride=5, feat_dtype=9, sh_deg=11, sh_act=5, bkgd_mode=abi.BKGD_PER_RAY, flags=-1)]
    for m in ok:
        assert l.selfocc_render_median(m, None) == 0, l.selfocc_last_error()
    bad = [(_args(depth=False, index=False), b"median_depth"), (_args(depth=False, index=False), b"median_index"),
           (_args(n_samples=0), b"n_samples"), (_args(n_samples=-3), b"n_samples"), (_args(n_rays=-1), b"n_rays"),
           (_args(sdf_vol=None), b"sdf_vol"), (_args(sample_pos=2), b"sample_pos"),
           (_args(jitter_mode=abi.JITTER_SINGLE), b"t_rand"), (_args(ray_mode=5), b"ray_mode")]
    for m, word in bad:
        assert l.selfocc_render_median(m, None) < 0, word
        err = l.selfocc_last_error()
        assert word in err, (word, err)
    assert l.selfocc_render_median(None, None) < 0 and b"args" in l.selfocc_last_error()


def _loop_reference(w, t):
    """the definition, one ray and one float32 addition at a time"""
    depth, index = [], []
    for wr, tr in zip(w, t):
        c, j = np.float32(0.0), len(wr) - 1
        for i, wi in enumerate(wr):
            c = np.float32(wi) if i == 0 else np.float32(c + np.float32(wi))
            if c >= np.float32(0.5):
                j = i
                break
        depth.append(tr[j]); index.append(j)
    return np.asarray(depth, dtype=np.float32), np.asarray(index, dtype=np.int32)


def _port_samples(kind, rays, cfg):
    vol, _ = mc.make_volume(kind)
    e = sy.explicit_rays(rays) if rays.pixel_grid else rays
    return tp.render_port(vol.mapping, vol.to_reference_layout(), 0, 0, e.origins, e.dirs, e.dir_norm, cfg,
                          t_rand=mc.t_rand_for(cfg, rays.n_rays), return_samples=True)


def test_reference_equals_a_plain_loop_on_port_weights():
    from selfocc_amd.render import median_depth_reference
    for kind, rays in (('linear', mc.make_pixel_rays('linear')), ('upscale', mc.make_explicit_rays('upscale'))):
        cfg = mc.make_cfg(mc.MAPPINGS[kind][1], 64, 20.0)
        s = _port_samples(kind, rays, cfg)
        depth, index = median_depth_reference(s['weights'], s['ts'])
        assert isinstance(depth, torch.Tensor) and depth.dtype == torch.float32 and index.dtype == torch.int32
        want_d, want_j = _loop_reference(s['weights'].numpy(), s['ts'].numpy())
        assert np.array_equal(index.numpy(), want_j) and np.array_equal(depth.numpy(), want_d)
        # arrays in, arrays out; leading dimensions are kept
        d2, j2 = median_depth_reference(s['weights'].numpy().reshape(2, -1, 64), s['ts'].numpy().reshape(2, -1, 64))
        assert isinstance(d2, np.ndarray) and d2.shape == (2, rays.n_rays // 2) and np.array_equal(j2.reshape(-1), want_j)
        assert mc.scene_is_sharp(want_j, s['weights'].numpy()) == [], (kind, mc.scene_stats(want_j, s['weights'].numpy()))


def test_scenes_are_sharp_in_every_gpu_case():
    """the conditions test_median_depth_gpu.py asserts on the GPU oracle hold on the CPU port of the same cases"""
    for name in mc.CASES:
        for pixel in (True, False):
            kind, rays, cfg, _ = mc.case(name, pixel)
            s = _port_samples(kind, rays, cfg)
            _, j = _loop_reference(s['weights'].numpy(), s['ts'].numpy())
            assert mc.scene_is_sharp(j, s['weights'].numpy()) == [], (name, pixel, mc.scene_stats(j, s['weights'].numpy()))


def test_reference_on_hand_made_rows():
    from selfocc_amd.render import median_depth_reference
    nan = float('nan')
    ts = np.arange(4, dtype=np.float32) + 10
    rows = [([0.7, 0.1, 0.1, 0.0], 0),            # crossing at sample 0
            ([0.25, 0.25, 0.3, 0.1], 1),          # c_1 == 0.5 exactly: >= counts (searchsorted side='left')
            ([0.1, 0.1, 0.1, 0.1], 3),            # never crossing: clamped to S - 1
            ([0.2, nan, 0.9, 0.9], 3),            # a NaN prefix never satisfies >=
            ([0.0, 0.0, 0.0, 0.5], 3)]            # crossing at the last sample
    w = np.asarray([r for r, _ in rows], dtype=np.float32)
    depth, index = median_depth_reference(w, np.repeat(ts[None], len(rows), 0))
    assert index.tolist() == [j for _, j in rows] and depth.tolist() == [10.0 + j for _, j in rows]
    # float32 accumulation, not double: (0.5 - 2^-25) + 2^-26 rounds to 0.5 in float32 and stays below it in double
    tiny = np.float32(2.0 ** -26)
    w32 = np.asarray([[0.25, 0.25 - 2.0 ** -25] + [tiny] * 6], dtype=np.float32)
    c32 = np.add.accumulate(w32, axis=-1, dtype=np.float32)
    c64 = np.cumsum(w32.astype(np.float64), axis=-1)
    j32 = int(np.argmax(c32 >= 0.5)) if (c32 >= 0.5).any() else 7
    j64 = int(np.argmax(c64 >= 0.5)) if (c64 >= 0.5).any() else 7
    assert j32 != j64                                               # the two accumulations part on this row ...
    assert median_depth_reference(w32, np.arange(8, dtype=np.float32)[None])[1].tolist() == [j32]   # ... and float32 is the rule
    # S = 1
    d1, j1 = median_depth_reference(torch.tensor([[0.9], [0.1], [nan]]), torch.tensor([[3.0], [4.0], [5.0]]))
    assert j1.tolist() == [0, 0, 0] and d1.tolist() == [3.0, 4.0, 5.0]


def test_render_median_depth_needs_device_tensors():
    import pytest
    from selfocc_amd.render import render_median_depth
    vol, aabb = mc.make_volume('linear')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_median_depth(vol, mc.make_explicit_rays('linear'), mc.make_cfg(aabb))


def test_head_accepts_the_flag_and_defaults_to_off():
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "head_occ_cfg.json")))['occ']
    assert 'return_median_depth' not in cfg
    assert MODELS.build(dict(type='NeuSHead', **cfg)).return_median_depth is False
    assert MODELS.build(dict(type='NeuSHead', return_median_depth=True, **cfg)).return_median_depth is True
