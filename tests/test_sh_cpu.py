"""CPU: spherical-harmonics colour (sh_deg 1 / 2, sh_act relu / sigmoid) — the host mirror against vectors produced by the
REAL reference (tests/golden/make_golden_sh.py -> sh.npz), the host-only argument checks of the C boundary, and the
construction rules of SDFVolume / SDFField / NeuSHead."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from kernel_report import HIPCC, kernels_of
from selfocc_amd import abi, sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sh.npz"))

SMALL_MAPPING = dict(nonlinear_mode='linear', h_size=[15, 0], h_range=[12.8, 0], h_half=True, w_size=[15, 0], w_range=[12.8, 0],
                     w_half=True, d_size=[3, 0], d_range=[-1.0, 2.0, 2.0])


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_sh_basis_vs_reference(deg):
    dirs = torch.tensor(GOLD['dirs'])
    assert dirs.shape[0] >= 180 and torch.allclose(dirs.norm(dim=-1), torch.ones(dirs.shape[0]), atol=1e-6)
    got = sh.sh_basis(deg, dirs)
    assert got.shape == (dirs.shape[0], (deg + 1) ** 2)
    assert torch.allclose(got, torch.tensor(GOLD[f'basis.{deg}']), rtol=1e-6, atol=1e-7)
    got64 = sh.sh_basis(deg, torch.tensor(GOLD['dirs64']))
    assert got64.dtype == torch.float64
    assert torch.allclose(got64, torch.tensor(GOLD[f'basis64.{deg}']), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("act", ['relu', 'sigmoid'])
@pytest.mark.parametrize("deg", [0, 1, 2])
def test_sh_colour_vs_reference_shrender(deg, act):
    """act(sum_k basis_k * f[c, k]) with colour-major coefficients == the reference's SHRender"""
    dirs, feat = torch.tensor(GOLD['dirs']), torch.tensor(GOLD[f'feat.{deg}'])
    ref = torch.tensor(GOLD[f'rgb.{deg}.{act}'])
    assert torch.allclose(sh.sh_colour(deg, act, dirs, feat), ref, rtol=1e-6, atol=1e-7)
    # spelled out, from the basis alone
    nb = (deg + 1) ** 2
    raw = (sh.sh_basis(deg, dirs)[:, None, :] * feat.view(-1, 3, nb)).sum(-1)
    col = torch.relu(raw + 0.5) if act == 'relu' else torch.sigmoid(raw)
    assert torch.allclose(col, ref, rtol=1e-6, atol=1e-7)
    # trailing pad channels of a stored row are not read
    padded = torch.cat([feat, torch.full((feat.shape[0], sh.feat_stride(deg) - feat.shape[1]), 1e6)], -1)
    assert torch.equal(sh.sh_colour(deg, act, dirs, padded), sh.sh_colour(deg, act, dirs, feat))


def test_sh_sizes():
    assert [sh.n_coef(d) for d in (0, 1, 2)] == [3, 12, 27]
    assert [sh.feat_stride(d) for d in (0, 1, 2)] == [4, 12, 28]
    with pytest.raises(ValueError, match="sh_deg 0, 1 and 2"):
        sh.sh_basis(3, torch.zeros(1, 3))
    with pytest.raises(ValueError, match="relu"):
        sh.check(1, 'tanh')


def test_render_args_layout_has_sh_fields_last(tmp_path):
    fields = [f for f, _ in abi.SoRenderArgs._fields_]
    assert fields[-3:] == ['inv_s_dev', 'sh_deg', 'sh_act']
    body = "\n".join(f'printf("%zu %zu\\n", sizeof(so_render_args), offsetof(so_render_args, {f}));' for f in ('sh_deg', 'sh_act'))
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/selfocc_hip.h"\n'
                   f'int main(void) {{ {body} printf("%d %d\\n", SO_SH_RELU, SO_SH_SIGMOID); return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    for f, line in zip(('sh_deg', 'sh_act'), lines):
        size, off = map(int, line.split())
        assert size == C.sizeof(abi.SoRenderArgs) and off == getattr(abi.SoRenderArgs, f).offset, f
    assert lines[2].split() == [str(abi.SH_RELU), str(abi.SH_SIGMOID)] == ['0', '1']
    assert abi.SoRenderArgs().sh_deg == 0 and abi.SoRenderArgs().sh_act == abi.SH_RELU       # zero = degree 0 with relu


def _args(**kw):
    """a launch that passes every check and, with n_rays = 0, returns before anything touches a device"""
    a = abi.SoRenderArgs()
    for ax, n in ((a.map.h, 32), (a.map.w, 32), (a.map.d, 4)):
        ax.tot_len, ax.size0, ax.range0 = n, float(n - 1), 12.8
    a.keep = C.create_string_buffer(64)          # never dereferenced
    a.sdf_vol = a.feat_vol = a.origins = a.dirs = C.addressof(a.keep)
    a.n_samples, a.n_rays, a.ray_mode = 32, 0, abi.RAYS_EXPLICIT
    a.n_rgb, a.n_sem, a.feat_dtype, a.feat_stride = 3, 0, abi.DTYPE_F32, 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_sh_argument_checks_are_pure_host_logic():
    """every refusal happens in so_validate_render, before any HIP call: rc < 0 and the key word in selfocc_last_error()"""
    from selfocc_amd._lib import lib
    l = lib()
    ok = [dict(), dict(sh_act=abi.SH_SIGMOID), dict(sh_deg=1, feat_stride=12), dict(sh_deg=2, feat_stride=28),
          dict(sh_deg=2, feat_stride=28, sh_act=abi.SH_SIGMOID), dict(n_rgb=3, n_sem=21, feat_stride=24)]
    for kw in ok:
        assert l.selfocc_render_fwd(_args(**kw), None) == 0, (kw, l.selfocc_last_error())
        ba = abi.SoRenderBwdArgs()
        ba.fwd = _args(**kw)
        assert l.selfocc_render_bwd(ba, None) == 0, (kw, l.selfocc_last_error())
    bad = [
        (dict(sh_deg=3, feat_stride=48), b"sh_deg"),
        (dict(sh_deg=-1), b"sh_deg"),
        (dict(sh_act=2), b"sh_act"),
        (dict(sh_deg=2, feat_stride=27), b"feat_stride"),
        (dict(sh_deg=2, feat_stride=32), b"feat_stride"),
        (dict(sh_deg=1, feat_stride=28), b"feat_stride"),
        (dict(sh_deg=2, feat_stride=48, n_sem=21), b"n_sem"),
        (dict(sh_act=abi.SH_SIGMOID, feat_stride=24, n_sem=21), b"n_sem"),
        (dict(sh_deg=2, feat_stride=28, feat_dtype=abi.DTYPE_BF16), b"bfloat16"),
    ]
    for kw, word in bad:
        assert l.selfocc_render_fwd(_args(**kw), None) < 0, kw
        err = l.selfocc_last_error()
        assert word in err, (kw, err)
        ba = abi.SoRenderBwdArgs()
        ba.fwd = _args(**kw)
        assert l.selfocc_render_bwd(ba, None) < 0 and word in l.selfocc_last_error(), kw


def test_sh_backward_workspace_uses_the_64_byte_record():
    """selfocc_render_bwd_ws_bytes: a spherical-harmonics sample is g_raw[3] + direction[3] + 8 geometry floats = the
    64-byte record of the 3-channel case at every degree (the brick kernel expands the basis), not a row of 27 products"""
    from selfocc_amd._lib import lib
    l = lib()
    ba = abi.SoRenderBwdArgs()
    for ax, n in ((ba.fwd.map.h, 257), (ba.fwd.map.w, 257), (ba.fwd.map.d, 25)):
        ax.tot_len = n
    ba.fwd.n_rays, ba.fwd.n_samples, ba.fwd.n_rgb, ba.fwd.n_sem = 28800, 256, 3, 0
    total = 28800 * 256
    plain = l.selfocc_render_bwd_ws_bytes(ba)
    assert total * 64 <= plain <= total * 64 + (8 << 20)
    for deg, act in ((2, abi.SH_RELU), (2, abi.SH_SIGMOID), (1, abi.SH_RELU), (0, abi.SH_SIGMOID)):
        ba.fwd.sh_deg, ba.fwd.sh_act = deg, act
        ws = l.selfocc_render_bwd_ws_bytes(ba)
        assert total * 64 <= ws <= total * 64 + (8 << 20) and ws % 256 == 0, (deg, act, ws)
        assert ws == plain
    ba.fwd.sh_deg = 3
    assert l.selfocc_render_bwd_ws_bytes(ba) == 0


def _field(color_dims, sh_deg, sh_act='relu', **kw):
    from selfocc_amd.model.head.neus_head import SDFField
    return SDFField(SMALL_MAPPING, embed_dims=16, color_dims=color_dims, density_layers=2, sh_deg=sh_deg, sh_act=sh_act, tpv=True, **kw)


@pytest.mark.parametrize("color_dims,sh_deg,sh_act", [(12, 1, 'relu'), (27, 2, 'relu'), (27, 2, 'sigmoid'), (3, 0, 'sigmoid')])
def test_field_and_head_construct_with_sh_colour(color_dims, sh_deg, sh_act):
    from selfocc_amd.model.head import NeuSHead
    from selfocc_amd.render import SDFVolume
    f = _field(color_dims, sh_deg, sh_act)
    assert (f.n_rgb, f.n_sem, f.sh_deg, f.sh_act) == (3, 0, sh_deg, sh_act)
    assert f.density_net[-1].out_features == 1 + color_dims
    assert f._feat_width() == SDFVolume.feat_width(3, 0, sh_deg) == sh.feat_stride(sh_deg)
    head = NeuSHead(roi_aabb=[0., 0., -1., 12.8, 12.8, 2.], num_samples=16, num_samples_importance=0, num_up_sample_steps=0,
                    use_numerical_gradients=False, ray_number=[4, 6], ray_img_size=[32, 48], mapping_args=SMALL_MAPPING,
                    embed_dims=16, color_dims=color_dims, density_layers=2, sh_deg=sh_deg, sh_act=sh_act, tpv=True)
    assert (head.model.field.sh_deg, head.model.field.sh_act) == (sh_deg, sh_act)
    # the dense volume of the op-by-op path has the kernels' layout: n_coef channels then zero padding
    H, W, D = f.size_h, f.size_w, f.size_d
    g = torch.Generator().manual_seed(0)
    rep = (torch.randn(1, H * W, 16, generator=g), torch.randn(1, D * H, 16, generator=g), torch.randn(1, W * D, 16, generator=g))
    with torch.no_grad():
        vol = f.pre_compute_density_color(rep)
    assert (vol.sh_deg, vol.sh_act, vol.n_rgb, vol.n_sem) == (sh_deg, sh_act, 3, 0)
    assert tuple(vol.feat.shape) == (H, W, D, sh.feat_stride(sh_deg))
    assert vol.feat[..., color_dims:].abs().max().item() == 0.0 if vol.feat.shape[-1] > color_dims else True
    assert vol.feat[..., :color_dims].abs().max().item() > 0.0


def test_default_sh_degree_constructs_with_27_colour_channels():
    """NeuSHead's own default is sh_deg=2: the documented defaults with color_dims=27 construct"""
    from selfocc_amd.model.head.neus_head import SDFField
    f = SDFField(SMALL_MAPPING, embed_dims=16, color_dims=27, tpv=True)
    assert (f.sh_deg, f.sh_act, f.n_rgb, f.n_sem) == (2, 'relu', 3, 0)
    f0 = SDFField(SMALL_MAPPING, embed_dims=16, color_dims=0, tpv=True)          # the depth configs: no colour, knobs unread
    assert (f0.n_rgb, f0.n_sem) == (0, 0)
    f24 = SDFField(SMALL_MAPPING, embed_dims=16, color_dims=24, sh_deg=0, tpv=True)   # the shipped occupancy configs
    assert (f24.sh_deg, f24.n_rgb, f24.n_sem) == (0, 3, 21)


def test_unbuilt_sh_combinations_are_refused_by_name():
    with pytest.raises(ValueError, match="pass sh_deg=0"):
        _field(3, 2)
    with pytest.raises(ValueError, match="pass sh_deg=0"):
        _field(24, 2)
    with pytest.raises(NotImplementedError, match="semantic channels are built with sh_deg=0"):
        _field(48, 2)
    with pytest.raises(NotImplementedError, match="semantic channels are built with sh_deg=0"):
        _field(24, 0, 'sigmoid')
    with pytest.raises(NotImplementedError, match="sh_deg 0, 1 and 2"):
        _field(48, 3)
    with pytest.raises(NotImplementedError, match="sh_deg 0, 1 and 2"):
        _field(75, 4)
    with pytest.raises(NotImplementedError, match="'relu' and 'sigmoid'"):
        _field(27, 2, 'tanh')
    with pytest.raises(NotImplementedError, match="float32"):
        _field(27, 2, feat_dtype=torch.bfloat16)


def test_volume_round_trips_through_the_reference_layout_with_sh():
    from selfocc_amd import synthetic as sy
    from selfocc_amd.render import SDFVolume
    v = sy.make_volume("cfg1", n_rgb=3, sh_deg=2, sh_act='sigmoid', seed=5)
    assert tuple(v.feat.shape[-1:]) == (28,) and v.feat[..., 27].abs().max().item() == 0.0 and v.n_colour == 27
    ref = v.to_reference_layout()
    assert tuple(ref.shape) == (1, 28, *v.sdf.shape)
    back = SDFVolume.from_reference_layout(v.mapping, ref, n_rgb=3, n_sem=0, sh_deg=2, sh_act='sigmoid')
    assert torch.equal(back.sdf, v.sdf) and torch.equal(back.feat, v.feat)
    assert (back.sh_deg, back.sh_act, back.n_rgb, back.n_sem) == (2, 'sigmoid', 3, 0)
    for w in (v.cpu(), v.to('cpu'), v.detached(), v.with_tensors(v.sdf, v.feat)):
        assert (w.sh_deg, w.sh_act, w.n_rgb, w.n_sem) == (2, 'sigmoid', 3, 0)
    # degree 0 keeps the layout it had
    v0 = sy.make_volume("cfg1", n_rgb=3, n_sem=5, seed=5)
    assert v0.feat.shape[-1] == 8 and (v0.sh_deg, v0.sh_act) == (0, 'relu')
    assert tuple(v0.to_reference_layout().shape) == (1, 9, *v0.sdf.shape)


def test_marshalling_carries_sh_fields():
    from selfocc_amd import synthetic as sy
    from selfocc_amd.render import marshal_render_args
    rays = sy.explicit_rays(sy.make_rays("cfg1"))
    cfg = sy.make_render_config("cfg1")
    a, out, _ = marshal_render_args(sy.make_volume("cfg1", n_rgb=3, sh_deg=2, sh_act='sigmoid'), rays, cfg)
    assert (a.sh_deg, a.sh_act, a.n_rgb, a.n_sem, a.feat_stride) == (2, abi.SH_SIGMOID, 3, 0, 28) and 'rgb' in out
    a, _, _ = marshal_render_args(sy.make_volume("cfg1", n_rgb=3, n_sem=5), rays, cfg)
    assert (a.sh_deg, a.sh_act, a.feat_stride) == (0, abi.SH_RELU, 8)


# ---- compiler report: the new forward kernels keep nothing in scratch ---------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
@pytest.mark.parametrize("src,base,count", [("render_fwd.hip", "render_fwd_explicit", 6), ("render_fwd.hip", "render_fwd_pixgrid", 6),
                                             ("render_train.hip", "render_fwd_samples_kernel", 18)],
                         # the ids these cases have always had: the names of the kernels before they became instances of `base`
                         ids=["render_fwd.hip-render_sh_explicit-6", "render_fwd.hip-render_sh_pixgrid-6",
                              "render_train.hip-render_sh_samples_kernel-18"])
def test_sh_forward_kernels_use_no_scratch(src, base, count):
    """eval forward (explicit / pixel grid x 3 basis sizes x 2 mapping kinds) and training forward (x 3 waves-per-ray forms):
    the folded gather keeps three sums, so nothing of width n_coef can spill"""
    hits = kernels_of(src, base, lambda r: r.nb > 0)
    assert len(hits) == count, [k.name for k in hits]
    assert sorted({(k.row.nb, k.row.nf) for k in hits}) == [(1, 4), (4, 12), (9, 28)]
    for k in hits:
        assert k.res["ScratchSize"] == 0, k
        assert k.res["VGPRs"] + k.res.get("AGPRs", 0) <= 256, k
