"""CPU: the host side of the sdf_loss term of ReprojLossMonoMultiNew — the so_reproj_pick_args layout against the
header, the entry points' refusals (before anything touches a device) and the loss class's constructor / argument errors."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from selfocc_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pick_args_layout_matches_header(tmp_path):
    fields = [f for f, _ in abi.SoReprojPickArgs._fields_]
    assert fields == ['weights', 'ts', 'deltas', 'values', 'pix', 'T_prev', 'T_next', 'R', 'S', 'img_h', 'img_w',
                      'pick_index', 'pick_value']
    body = "\n".join(f'printf("%zu %zu\\n", sizeof(so_reproj_pick_args), offsetof(so_reproj_pick_args, {f}));' for f in fields)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/selfocc_hip.h"\n'
                   f'int main(void) {{ {body} printf("%zu %d\\n", sizeof(so_reproj_args), SELFOCC_ABI_VERSION); return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    for f, line in zip(fields, lines):
        size, off = map(int, line.split())
        assert size == C.sizeof(abi.SoReprojPickArgs) and off == getattr(abi.SoReprojPickArgs, f).offset, f
    # entry points only: the existing struct and the ABI version are where they were
    size, version = map(int, lines[len(fields)].split())
    assert size == C.sizeof(abi.SoReprojArgs)
    assert version == abi.ABI_VERSION == 35


def _args(**kw):
    """passes every check and, with R = 0, returns before anything touches a device"""
    a = abi.SoReprojPickArgs()
    a.keep = C.create_string_buffer(64)          # never dereferenced
    for f in ('weights', 'ts', 'deltas', 'values', 'pix', 'T_prev', 'T_next', 'pick_index', 'pick_value'):
        setattr(a, f, C.addressof(a.keep))
    a.R, a.S, a.img_h, a.img_w = 0, 12, 48.0, 100.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_pick_entry_refusals_are_pure_host_logic():
    from selfocc_amd._lib import lib
    l = lib()
    assert l.selfocc_abi_version() == 35
    assert l.selfocc_reproj_pick_fwd(_args(), None) == 0
    assert l.selfocc_reproj_pick_fwd(_args(deltas=None), None) == 0          # deltas is optional
    assert l.selfocc_reproj_pick_fwd(_args(S=1), None) == 0 and l.selfocc_reproj_pick_fwd(_args(S=512), None) == 0
    cases = [(dict(S=0), b"1 <= S <= 512"), (dict(S=513), b"1 <= S <= 512"), (dict(R=-1), b"R >= 0"),
             (dict(img_h=0.0), b"image size")]
    cases += [({f: None}, b"NULL input") for f in ('weights', 'ts', 'values', 'pix', 'T_prev', 'T_next')]
    cases += [({f: None}, b"NULL output") for f in ('pick_index', 'pick_value')]
    for kw, word in cases:
        rc = l.selfocc_reproj_pick_fwd(_args(**kw), None)
        err = l.selfocc_last_error()
        assert rc < 0 and b"reproj_pick" in err and word in err, (kw, rc, err)
    assert l.selfocc_reproj_pick_fwd(None, None) < 0
    keep = C.create_string_buffer(64)
    p = C.addressof(keep)
    assert l.selfocc_reproj_pick_bwd(p, p, p, 0, 12, None) == 0
    for (pi, g, out, S), word in (((p, p, p, 0), b"1 <= S <= 512"), ((p, p, p, 513), b"1 <= S <= 512"),
                                  ((None, p, p, 12), b"NULL"), ((p, None, p, 12), b"NULL"), ((p, p, None, 12), b"NULL")):
        rc = l.selfocc_reproj_pick_bwd(pi, g, out, 0, S, None)
        err = l.selfocc_last_error()
        assert rc < 0 and b"reproj_pick_bwd" in err and word in err, (S, rc, err)


def _loss(**kw):
    from selfocc_amd.registry import OPENOCC_LOSS
    import selfocc_amd.loss  # noqa: F401
    return OPENOCC_LOSS.build(dict(type='ReprojLossMonoMultiNew', weight=1.0, img_size=[48, 100], **kw))


def _inputs(R=6, S=4):
    import numpy as np
    eye = np.eye(4)[None]
    return dict(curr_imgs=torch.rand(1, 1, 3, 48, 100), prev_imgs=torch.rand(1, 1, 3, 48, 100),
                next_imgs=torch.rand(1, 1, 3, 48, 100), ray_indices=[torch.arange(R).repeat_interleave(S)],
                weights=[torch.rand(R * S)], ts=[torch.rand(R * S) + 1], metas=[dict(img2prevImg=eye, img2nextImg=eye)],
                ms_rays=torch.rand(R, 2) * 40, sample_sdf=[torch.randn(R * S)])


def test_constructor_and_input_dict():
    on = _loss(sdf_loss=True)
    assert on.sdf_loss is True and on.sdf_loss_weight == 0.1                 # the reference's default weight
    assert on.input_dict['sample_sdfs'] == 'sample_sdf'                       # the head's key, under the reference's parameter name
    assert _loss(sdf_loss=True, sdf_loss_weight=0.25).sdf_loss_weight == 0.25
    off = _loss()
    assert off.sdf_loss is False and 'sample_sdfs' not in off.input_dict
    keys = dict(off.input_dict)
    assert _loss(sdf_loss=True, input_dict=keys).input_dict == keys           # an explicit dict is taken as given


def test_missing_sample_sdfs_raises_by_name():
    keys = dict(_loss().input_dict)                                           # no 'sample_sdfs' entry
    with pytest.raises(ValueError, match="sample_sdfs"):
        _loss(sdf_loss=True, input_dict=keys)(_inputs())
    # the default dict reads the head's key: a head without return_sample_sdf has none
    inp = _inputs()
    del inp['sample_sdf']
    with pytest.raises(KeyError, match="sample_sdf"):
        _loss(sdf_loss=True)(inp)


def test_ray_sharded_head_with_sdf_loss_raises_by_name():
    from selfocc_amd.dist import LocalRows
    inp = _inputs()
    shard = object()                                                          # only its presence is looked at
    for k in ('weights', 'ts', 'ray_indices', 'sample_sdf'):
        inp[k] = LocalRows(inp[k], shard)
    with pytest.raises(NotImplementedError, match=r"sdf_loss=True.*ray-sharded"):
        _loss(sdf_loss=True)(inp)
