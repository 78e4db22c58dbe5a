"""GPU: render, train and query any semantic class count from 2 to 21.

Every volume here has 64.0 in its pad channels (nsem_cases.volume); the logits are N(0, 1), so a pad channel that reached a
soft-max, a sum or a gradient row would take it over.  Class counts 2, 4, 6, 11, 16, 17, 20 cover pad sizes 0 - 3 and both ends
of every row width (8, 12, 16, 20, 24 floats); 5 and 21 are the controls that run the kernels of every earlier version.

Which case reaches which built route.  The kernels are the render templates instantiated on a masked row, R = so_row<NF, false,
0, true> of csrc/render_row.h (NF = the row width):
  render_fwd_pixgrid / render_fwd_explicit <R, Canonical>        test_exact_launches_vs_oracle (every class count),
                                                                 test_single_jitter_..., test_two_segment_mapping_...,
                                                                 test_rays_entering_from_outside_the_box[exact]
  render_fwd_pixgrid / render_fwd_explicit <R, CanonicalUpscale> test_linear_upscale_mapping_vs_float64_port, ..._at_every_row_width
  render_fwd_explicit <R, FastFaceSafe> (direct gathers)         test_default_flags_vs_oracle (explicit launch)
  render_fwd_pixgrid <R, FastFaceSafe> (LDS-staged block,        test_default_flags_vs_oracle (pixel grid), test_sample_at_mid_...,
      semantic sums in LDS at NF >= 20)                          test_rays_entering_...[fast] (clamped / zero-padded gathers),
                                                                 test_launch_large_enough_for_the_brick_repack (with the brick)
  render_fwd_samples_kernel <R, 1 / 2 / 4 waves per ray, linear> test_training_forward_... (S = 32 / 100 / 256)
  render_fwd_samples_kernel <R, ., upscale>                      test_linear_upscale_mapping_vs_float64_port (per-sample launch)
  render_bwd_kernel <R, M, WPR, atomic / binned, linear>         test_backward_vs_float64_autograd (S = 32: M 1, WPR 1; S = 100: M 2,
                                                                 WPR 1), test_backward_binned_vs_atomic_at_the_auto_threshold
                                                                 (S = 256: M 1, WPR 4)
  render_bwd_kernel <R, ., ., ., upscale>                        test_linear_upscale_mapping_vs_float64_port (binned against atomic)
  rb_brick_kernel <so_row<12 / 16 / 20, false>> (the unmasked    every binned case above
      row of the width; 8 / 24 shared with 5 / 21 classes)
  SDFField / NeuSHead with 20 (and 6) classes                    test_head_with_20_classes_*, test_fused_and_op_by_op_field_routes_agree
"""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import torch_port as tp
from selfocc_amd import abi, synthetic as sy
from selfocc_amd.render import RaySet, RenderConfig, SDFVolume, render_rays, render_rays_autograd
from nsem_cases import CLASS_COUNTS, CONTROLS, PAD, fill_pad, stride, volume
from test_render_gpu import _cmp, parity_report

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
# sum_k sem_k == acc: the soft-max sums to 1 within n_sem roundings, the composite adds S terms:
# (n_sem + S) * 2^-23 <= (21 + 256) * 1.2e-7 = 3.3e-5 at the largest case used here
SUM_TOL = 5e-5


def _dev(r):
    if r.pixel_grid:
        return RaySet(img2lidar=r.img2lidar.to(D0), nx=r.nx, ny=r.ny, sx=r.sx, sy=r.sy, ox=r.ox, oy=r.oy)
    return RaySet(origins=r.origins.to(D0), dirs=r.dirs.to(D0), dir_norm=None if r.dir_norm is None else r.dir_norm.to(D0))


def _sem_sums_to_acc(ref, got, n_sem):
    assert (ref['acc'] > 0.05).sum() > 100                    # not a test of the background
    assert tuple(got['sem'].shape) == tuple(ref['sem'].shape) == (ref['acc'].shape[0], n_sem)
    assert (ref['sem'].sum(-1) - ref['acc']).abs().max() <= SUM_TOL          # the reference itself stays inside
    assert (got['sem'].cpu().sum(-1) - got['acc'].cpu()).abs().max() <= SUM_TOL


_REF = {}


def _cfg1_ref(n_sem, exact):
    """volume, rays and the oracle's outputs of the cfg1 frame: computed once per (class count, mode), never modified"""
    key = (n_sem, exact)
    if key not in _REF:
        vol = volume("cfg1", n_sem, seed=3)
        rays = sy.make_rays("cfg1", seed=3)
        cfg = sy.make_render_config("cfg1", inv_s=20.0, bkgd_mode=abi.BKGD_CONST, bkgd=(1.0, 0.5, 0.25), clamp_rgb=True, exact=exact)
        _REF[key] = (vol, rays, cfg, oracle.render_fwd(vol, rays, cfg))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# eval forward against the C oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sem", CLASS_COUNTS + CONTROLS)
def test_exact_launches_vs_oracle(hip, n_sem):
    vol, rays, cfg, ref = _cfg1_ref(n_sem, True)
    got = render_rays(vol.to(D0), _dev(rays), cfg)
    _cmp(got, ref)
    _sem_sums_to_acc(ref, got, n_sem)
    got_x = render_rays(vol.to(D0), _dev(sy.explicit_rays(rays)), cfg)
    _cmp(got_x, ref)
    _sem_sums_to_acc(ref, got_x, n_sem)


@pytest.mark.parametrize("n_sem", CLASS_COUNTS + CONTROLS)
def test_default_flags_vs_oracle(hip, n_sem):
    vol, rays, cfg, ref = _cfg1_ref(n_sem, False)
    res = []
    for r in (rays, sy.explicit_rays(rays)):
        got = {k: t.clone() for k, t in render_rays(vol.to(D0), _dev(r), cfg).items()}
        rep = parity_report(got, ref, label=f"cfg1 n_sem={n_sem} {'pixel grid' if r.pixel_grid else 'explicit'}")
        assert rep['sem_max_abs'] <= 1e-4 and rep['sem_frac'] >= 0.995         # sem under the rgb rule
        _sem_sums_to_acc(ref, got, n_sem)
        res.append(got)
    # SO_FLAG_NO_FACE_SAFE is an A/B switch of the shipped widths: a masked launch ignores it and marches face-safe
    if n_sem not in CONTROLS:
        from dataclasses import replace
        got_n = render_rays(vol.to(D0), _dev(rays), replace(cfg, face_safe=False))
        for k in got_n:
            assert torch.equal(got_n[k], res[0][k]), k


def test_single_jitter_takes_the_canonical_route(hip):
    n_sem = 6
    vol = volume("cfg1", n_sem, seed=4)
    ex = sy.explicit_rays(sy.make_rays("cfg1", seed=4))
    cfg = sy.make_render_config("cfg1", jitter_mode=abi.JITTER_SINGLE, bkgd_mode=abi.BKGD_PER_RAY)
    g = torch.Generator().manual_seed(0)
    t_rand, bk = torch.rand(ex.n_rays, generator=g), torch.rand(ex.n_rays, 3, generator=g)
    ref = oracle.render_fwd(vol, ex, cfg, t_rand=t_rand, bkgd_rays=bk)
    got = render_rays(vol.to(D0), _dev(ex), cfg, t_rand=t_rand.to(D0), bkgd_rays=bk.to(D0))
    _cmp(got, ref)
    _sem_sums_to_acc(ref, got, n_sem)


def test_sample_at_mid_default_flags(hip):
    n_sem = 11
    vol = volume("cfg1", n_sem, seed=5)
    rays = sy.make_rays("cfg1", seed=5)
    cfg = sy.make_render_config("cfg1", inv_s=20.0, sample_pos=1)
    ref = oracle.render_fwd(vol, rays, cfg)
    got = render_rays(vol.to(D0), _dev(rays), cfg)
    parity_report(got, ref, label="cfg1 n_sem=11 sample_pos=1")
    _sem_sums_to_acc(ref, got, n_sem)
    got_e = render_rays(vol.to(D0), _dev(rays), sy.make_render_config("cfg1", inv_s=20.0, sample_pos=1, exact=True))
    _cmp(got_e, ref)


def test_two_segment_mapping_takes_the_canonical_route(hip):
    from selfocc_amd.mapping import GridMeterMapping
    n_sem = 16
    m = GridMeterMapping(nonlinear_mode='linear', h_size=[6, 3], h_range=[6.0, 9.0], h_half=False,
                         w_size=[6, 3], w_range=[6.0, 9.0], w_half=False, d_size=[4, 2], d_range=[-1.0, 3.0, 7.0])
    g = torch.Generator().manual_seed(0)
    sdf = 0.3 * torch.randn(m.size_h, m.size_w, m.size_d, generator=g)
    feat = torch.full((m.size_h, m.size_w, m.size_d, stride(n_sem)), PAD)
    feat[..., :3 + n_sem] = torch.randn(m.size_h, m.size_w, m.size_d, 3 + n_sem, generator=g)
    vol = SDFVolume(m, sdf.contiguous(), feat.contiguous(), 3, n_sem)
    o = torch.tensor([[0.3, -0.2, 1.0]]).repeat(500, 1)
    dirs = torch.nn.functional.normalize(torch.randn(500, 3, generator=g), dim=-1)
    rays = RaySet(origins=o.contiguous(), dirs=dirs.contiguous(), dir_norm=torch.ones(500))
    cfg = RenderConfig(aabb=(-15.0, -15.0, -1.0, 15.0, 15.0, 7.0), n_samples=48, inv_s=5.0)
    ref = oracle.render_fwd(vol, rays, cfg, per_sample=True, want_grad_samples=True)
    got = render_rays(vol.to(D0), _dev(rays), cfg)                          # eval launch: render_fwd_explicit<so_row<20, false, 0, true>, Canonical>
    _cmp(got, ref, keys=list(got))
    _sem_sums_to_acc(ref, got, n_sem)
    got_t = render_rays(vol.to(D0), _dev(rays), cfg, per_sample=True, want_grad_samples=True)
    assert torch.equal(got_t['sdf'].cpu(), ref['sdf'])
    _cmp(got_t, ref)


@pytest.mark.parametrize("exact", [True, False])
def test_rays_entering_from_outside_the_box(hip, exact):
    """the setup of tests/test_render_gpu.py::test_rays_entering_from_outside_the_box: clamped and zero-padded gathers"""
    n_sem = 20
    vol = volume("cfg1", n_sem, seed=9)
    rays = sy.make_rays("cfg1", seed=9)
    M = rays.img2lidar.clone().repeat(3, 1, 1)
    M[0, :3, 3] += torch.tensor([-9.0, 0.3, 0.2])
    M[1, :3, 3] += torch.tensor([-3.0, -8.5, 0.4])
    M[2, :3, 3] += torch.tensor([-30.0, 40.0, 9.0])
    rays.img2lidar = M
    cfg = sy.make_render_config("cfg1", inv_s=20.0, exact=exact)
    ref = oracle.render_fwd(vol, rays, cfg)
    assert (ref['nears'] > 0).float().mean() > 0.5
    got = render_rays(vol.to(D0), _dev(rays), cfg)
    if exact:
        _cmp(got, ref)
    else:
        parity_report(got, ref, label="cfg1-entering n_sem=20")
    _sem_sums_to_acc(ref, got, n_sem)
    if not exact:                                                            # and the direct (not staged) gathers
        got_x = render_rays(vol.to(D0), _dev(sy.explicit_rays(rays)), cfg)
        parity_report(got_x, ref, label="cfg1-entering n_sem=20 explicit")


@pytest.mark.parametrize("n_sem", [20, 11])
def test_launch_large_enough_for_the_brick_repack(hip, n_sem):
    """cfg2 volume, 6 x 800 x 17 rays x 128 samples: just past the 16 x voxels rule of render_rays, so the launch re-packs the SDF
    volume and the staged pixel-grid kernel reads the brick records"""
    vol = volume("cfg2", n_sem, seed=0)
    rays = sy.make_rays("cfg2", seed=0)
    sub = RaySet(img2lidar=rays.img2lidar, nx=rays.nx, ny=17, sx=rays.sx, sy=rays.sy, oy=rays.sy * 200)
    cfg = sy.make_render_config("cfg2", inv_s=20.0)
    assert 16 * vol.sdf.numel() <= sub.n_rays * cfg.n_samples < 17 * vol.sdf.numel()
    ref = oracle.render_fwd(vol, sub, cfg)
    from selfocc_amd import render as R
    got = render_rays(vol.to(D0), _dev(sub), cfg)
    assert any(k[2] == tuple(vol.sdf.shape) for k in R._BRICK_WS)             # the launch took a brick workspace of this shape
    parity_report(got, ref, label=f"cfg2 brick n_sem={n_sem}")
    _sem_sums_to_acc(ref, got, n_sem)


def _upscale_vs_float64_port(n_sem):
    """scene, rays and the off-face ray rule of tests/test_mapping_upscale_gpu.py (the C oracle has no upscale mapping: the
    reference is the float64 port); eval launch on explicit rays and pixel grid, the per-sample launch, binned against atomic"""
    import test_mapping_upscale_gpu as up
    from selfocc_amd.mapping import GridMeterMapping
    m = GridMeterMapping(**up.HEAD_UPSCALE)
    vol = fill_pad(up._volume(m, 3, n_sem))
    assert vol.feat.shape[-1] == stride(n_sem)
    cfg = RenderConfig(aabb=up.AABB, n_samples=64, inv_s=20.0, sample_pos=abi.SAMPLE_AT_START)
    pix = up._pixel_rays()
    ex, idx = up._off_faces(m, sy.explicit_rays(pix), cfg, 1e-3)
    assert idx.numel() >= 300
    up._coverage(m, ex, cfg)
    dd = torch.float64
    ref = tp.render_port(m.mapping, vol.to_reference_layout().to(dd), 3, n_sem, ex.origins.to(dd), ex.dirs.to(dd), ex.dir_norm.to(dd), cfg)
    ref = {k: v.float() for k, v in ref.items()}
    v = vol.to(D0)
    got = render_rays(v, _dev(ex), cfg)
    parity_report(got, ref, label=f"upscale explicit n_sem={n_sem}")
    _sem_sums_to_acc(ref, got, n_sem)
    gp = render_rays(v, _dev(pix), cfg)
    parity_report({k: t[idx.to(D0)] for k, t in gp.items()}, ref, label=f"upscale pixel grid n_sem={n_sem}")
    gt = render_rays(v, _dev(ex), cfg, per_sample=True)
    parity_report({k: gt[k] for k in got}, ref, label=f"upscale per-sample launch n_sem={n_sem}")
    res = {}
    for mode in ("atomic", "binned"):
        cfg.bwd_scatter = mode
        sdf, feat = v.sdf.clone().requires_grad_(True), v.feat.clone().requires_grad_(True)
        inv_s = torch.tensor([20.0], device=D0, requires_grad=True)
        out = render_rays_autograd(SDFVolume(m, sdf, feat, 3, n_sem), inv_s, _dev(ex), cfg)
        (out['depth'].mean() + out['rgb'].mean() + out['sem'].square().mean() + out['sdf'].abs().mean()).backward()
        res[mode] = (sdf.grad, feat.grad)
        assert feat.grad[..., 3:3 + n_sem].abs().max() > 0
        if stride(n_sem) > 3 + n_sem:
            assert feat.grad[..., 3 + n_sem:].abs().max() == 0
    for a, b in zip(res["atomic"], res["binned"]):
        assert _rel_l2(b.double(), a.double()) < 1e-5 and (b - a).abs().max() <= 1e-4 * a.abs().max()


def test_linear_upscale_mapping_vs_float64_port(hip):
    """6 classes: the 12-float masked row"""
    _upscale_vs_float64_port(6)


@pytest.mark.parametrize("n_sem", [4, 11, 17, 20, 5])
def test_linear_upscale_mapping_at_every_row_width(hip, n_sem):
    """one class count for each other masked row width (8, 16, 20, 24 floats) and the 5-class control (the unmasked 8-float row)"""
    _upscale_vs_float64_port(n_sem)


# ---------------------------------------------------------------------------------------------------------------------------------
# training forward (per-sample outputs): 1 / 2 / 4 waves per ray
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sem,S", [(2, 32), (6, 100), (11, 256), (16, 32), (17, 100), (20, 256), (4, 256), (20, 32)])
def test_training_forward_vs_oracle_and_the_sdf_only_launch(hip, n_sem, S):
    vol = volume("cfg1", n_sem, seed=7)
    rays = sy.make_rays("cfg1", seed=7)
    cfg = sy.make_render_config("cfg1", inv_s=20.0)
    cfg.n_samples = S
    ref = oracle.render_fwd(vol, rays, cfg, per_sample=True, want_grad_samples=True)
    got = render_rays(vol.to(D0), _dev(rays), cfg, per_sample=True, want_grad_samples=True)
    _cmp(got, ref)                                            # rgb and sem among them
    _sem_sums_to_acc(ref, got, n_sem)
    bare = render_rays(SDFVolume(vol.mapping, vol.sdf.to(D0)), _dev(rays), cfg, per_sample=True, want_grad_samples=True)
    for k in ('weights', 'ts', 'deltas', 'sdf', 'grad', 'depth', 'acc'):
        assert torch.equal(got[k], bare[k]), k                # the geometry does not depend on the colour / semantic channels


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("scatter", ["atomic", "binned"])
@pytest.mark.parametrize("n_sem,S", [(n, s) for n in (2, 6, 11, 17, 20) for s in (32, 100)])
def test_backward_vs_float64_autograd(hip, n_sem, S, scatter):
    """body and bounds of tests/test_render_bwd_gpu.py::test_render_backward_vs_float64_autograd, with its scene, rays and
    its jitter at each S (per-bin at 32, none at 100).  The SDF volume, hence every sample position, is the same for every
    class count (make_volume draws the SDF before the channels), so the per-sample `grad` — piece-wise constant per cell, and
    therefore one cell off in float64 wherever a float32 sample sits within rounding of a voxel face — compares as it does there."""
    n_rgb = 3
    vol = volume("cfg1", n_sem, seed=11, noise=0.02)
    ex = sy.explicit_rays(sy.make_rays("cfg1", seed=11))
    jitter = abi.JITTER_PER_BIN if S == 32 else abi.JITTER_NONE
    cfg = sy.make_render_config("cfg1", inv_s=12.0, jitter_mode=jitter, bkgd_mode=abi.BKGD_PER_RAY)
    cfg.n_samples, cfg.bwd_scatter = S, scatter
    N = ex.n_rays
    g = torch.Generator().manual_seed(3)
    t_rand = None if jitter == abi.JITTER_NONE else torch.rand(N, S + 1, generator=g)
    bk = torch.rand(N, 3, generator=g)
    G = dict(depth=torch.randn(N, generator=g), acc=torch.randn(N, generator=g), weights=torch.randn(N, S, generator=g),
             sdf=0.1 * torch.randn(N, S, generator=g), grad=0.1 * torch.randn(N, S, 3, generator=g),
             rgb=torch.randn(N, 3, generator=g), sem=torch.randn(N, n_sem, generator=g))
    dd = torch.float64
    vol64 = vol.to_reference_layout()[0].to(dd).requires_grad_(True)      # (1 + 3 + n_sem, H, W, D): no pad
    inv_s64 = torch.tensor(cfg.inv_s, dtype=dd, requires_grad=True)
    ref = tp.render_port_differentiable(vol.mapping, vol64, n_rgb, n_sem, ex.origins.to(dd), ex.dirs.to(dd), ex.dir_norm.to(dd), cfg,
                                        inv_s64, None if t_rand is None else t_rand.to(dd), bk.to(dd))
    sum((ref[k] * G[k].to(dd)).sum() for k in G).backward()
    ref_gsdf, ref_gfeat = vol64.grad[0], vol64.grad[1:].permute(1, 2, 3, 0)

    v = vol.to(D0)
    sdf_p, feat_p = v.sdf.clone().requires_grad_(True), v.feat.clone().requires_grad_(True)
    inv_s = torch.tensor([cfg.inv_s], device=D0, requires_grad=True)
    out = render_rays_autograd(SDFVolume(v.mapping, sdf_p, feat_p, n_rgb, n_sem), inv_s, _dev(ex), cfg, want_grad_samples=True,
                               t_rand=None if t_rand is None else t_rand.to(D0), bkgd_rays=bk.to(D0))
    for k in G:
        assert torch.allclose(out[k].detach().cpu().double(), ref[k].detach(), rtol=2e-3, atol=2e-4), k
    sum((out[k] * G[k].to(D0)).sum() for k in G).backward()
    e_sdf = _rel_l2(sdf_p.grad.cpu().double(), ref_gsdf)
    e_f = _rel_l2(feat_p.grad.cpu().double()[..., :n_rgb + n_sem], ref_gfeat)
    e_s = abs(inv_s.grad.item() - inv_s64.grad.item()) / (abs(inv_s64.grad.item()) + 1e-12)
    print(f"\n[nsem bwd] n_sem={n_sem} S={S} {scatter}: sdf {e_sdf:.3e} feat {e_f:.3e} inv_s {e_s:.3e}")
    assert e_sdf < 2e-3, f"d/d sdf_vol rel L2 {e_sdf:.3e}"
    assert (sdf_p.grad.cpu().double() - ref_gsdf).abs().max() < 2e-2 * ref_gsdf.abs().max()
    assert e_f < 2e-3, f"d/d feat_vol rel L2 {e_f:.3e}"
    assert feat_p.shape[-1] == stride(n_sem)
    if stride(n_sem) > n_rgb + n_sem:
        assert feat_p.grad[..., n_rgb + n_sem:].abs().max() == 0          # exactly: nothing is ever added to a pad channel
    assert feat_p.grad[..., n_rgb + n_sem - 1].abs().max() > 0
    assert e_s < 5e-2, f"d/d inv_s rel {e_s:.3e} ({inv_s.grad.item()} vs {inv_s64.grad.item()})"


@pytest.mark.parametrize("scatter", ["atomic", "binned"])
def test_backward_zero_upstream_gives_zero_gradients(hip, scatter):
    n_sem = 11
    vol = volume("cfg1", n_sem, seed=1).to(D0)
    ex = sy.explicit_rays(sy.make_rays("cfg1", seed=1))
    sdf_p, feat_p = vol.sdf.clone().requires_grad_(True), vol.feat.clone().requires_grad_(True)
    inv_s = torch.tensor([20.0], device=D0, requires_grad=True)
    cfg = sy.make_render_config("cfg1")
    cfg.bwd_scatter = scatter
    out = render_rays_autograd(SDFVolume(vol.mapping, sdf_p, feat_p, 3, n_sem), inv_s, _dev(ex), cfg)
    ((out['depth'].sum() + out['sem'].sum() + out['rgb'].sum() + out['weights'].sum()) * 0.0).backward()
    assert sdf_p.grad.abs().max() == 0 and feat_p.grad.abs().max() == 0 and inv_s.grad.abs().max() == 0


@pytest.mark.parametrize("n_sem", [6, 17])
def test_backward_binned_vs_atomic_at_the_auto_threshold(hip, n_sem):
    """the smallest launch bwd_scatter='auto' sends to the binned scatter: 2^19 samples = 2 048 rays x 256, on the 257 x 257 x 25
    volume; bounds of tests/test_render_bwd_gpu.py::test_render_backward_binned_vs_atomic_at_training_shape"""
    vol = volume("cfg5", n_sem, seed=2).to(D0)
    full = sy.explicit_rays(sy.make_rays("cfg5", seed=2))
    idx = torch.linspace(0, full.n_rays - 1, 2048).long()
    ex = _dev(RaySet(origins=full.origins[idx].contiguous(), dirs=full.dirs[idx].contiguous(), dir_norm=full.dir_norm[idx].contiguous()))
    res = {}
    for mode in ("atomic", "auto"):
        cfg = sy.make_render_config("cfg5")
        cfg.bwd_scatter = mode
        assert ex.n_rays * cfg.n_samples == 1 << 19
        inv_s = torch.tensor([float(cfg.inv_s)], device=D0, requires_grad=True)
        sdf, feat = vol.sdf.clone().requires_grad_(True), vol.feat.clone().requires_grad_(True)
        out = render_rays_autograd(SDFVolume(vol.mapping, sdf, feat, 3, n_sem), inv_s, ex, cfg)
        loss = out['depth'].mean() + out['sdf'].abs().mean() * 0.1 + (out['grad'].norm(dim=-1) - 1).square().mean() * 0.1 + \
            (out['weights'] * torch.linspace(0, 1, out['weights'].shape[-1], device=D0)).sum(-1).mean() + out['rgb'].mean() + \
            out['sem'].square().mean()
        loss.backward()
        res[mode] = (sdf.grad, feat.grad, inv_s.grad)
        if stride(n_sem) > 3 + n_sem:                                        # 6 classes: 3 pad channels; 17 fill their row
            assert feat.grad[..., 3 + n_sem:].abs().max() == 0
    a, b = res["atomic"], res["auto"]
    for k in (0, 1):
        assert a[k].abs().max() > 0
        assert _rel_l2(b[k].double(), a[k].double()) < 1e-5
        assert (b[k] - a[k]).abs().max() <= 1e-4 * a[k].abs().max()
    assert abs(b[2].item() - a[2].item()) <= 1e-3 * abs(a[2].item()) + 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# the head: 20 classes (color_dims = 23), the fused field route
# ---------------------------------------------------------------------------------------------------------------------------------
MAP = sy.CONFIGS["cfg1"]["mapping"]
AABB = list(sy.CONFIGS["cfg1"]["aabb"])
C = 96                                   # the embedding width the fused training route of the field is built for


def _head(color_dims=23, **kw):
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model, selfocc_amd.loss  # noqa: F401
    cfg = dict(type='NeuSHead', roi_aabb=AABB, resolution=0.4, near_plane=0.0, far_plane=1e10, num_samples=32,
               num_samples_importance=0, num_up_sample_steps=0, base_variance=4, beta_init=0.25, beta_hand_tune=False,
               use_numerical_gradients=False, sample_gradient=True, return_uniform_sdf=False, return_second_grad=True,
               return_sem=True, ray_sample_mode='cellular', ray_number=[6, 10], ray_img_size=[64, 64],
               trans_kw='temImg2lidar', render_bkgd='random', mapping_args=MAP, embed_dims=C, color_dims=color_dims,
               density_layers=2, sh_deg=0, sh_act='relu', two_split=False, tpv=True, return_max_depth=True)
    cfg.update(kw)
    torch.manual_seed(0)
    head = MODELS.build(cfg).to(D0)
    with torch.no_grad():
        head.model.field.density_net[-1].bias[0] = -0.25       # the SDF of _inputs' planes changes sign inside the box
    return head


def _inputs(n_sem, n_cams=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    H, W, Z = 32, 32, 4
    rep = [(0.3 * torch.randn(1, n, C, generator=g)).to(D0).requires_grad_(True) for n in (H * W, Z * H, W * Z)]
    cams = sy.make_cameras("cfg1", seed).repeat(n_cams, 1, 1).clone()
    cams[1:, :3, 3] += torch.tensor([0.5, -0.3, 0.0])
    metas = [dict(temImg2lidar=cams.numpy(), img2lidar=cams.numpy(), img_shape=(64, 64),
                  sem=torch.randint(0, n_sem, (n_cams, 64, 64), generator=g).numpy())]
    imgs = torch.rand(1, n_cams, 3, 64, 64, generator=g).to(D0)
    return rep, metas, imgs


def test_head_with_20_classes_trains(hip):
    from selfocc_amd.registry import OPENOCC_LOSS
    os.environ['eval'] = 'false'
    head = _head().train()
    f = head.model.field
    assert (f.n_rgb, f.n_sem, f._feat_width()) == (3, 20, 24)
    rep, metas, imgs = _inputs(20)
    np.random.seed(0)
    out = head(rep, metas, global_iter=0)
    assert out['sem'][0].shape == (1, 2, 60, 20) and tuple(f.volume.feat.shape) == (32, 32, 4, 24)
    assert f.volume.feat[..., 23].abs().max() == 0 and f.volume.feat[..., 22].abs().max() > 0
    loss_fn = OPENOCC_LOSS.build(dict(type='MultiLoss', loss_cfgs=[
        dict(type='SemCELossMS', weight=1.0, img_size=[64, 64], ray_resize=[6, 10],
             input_dict={'sem': 'sem', 'metas': 'metas', 'ms_rays': 'ms_rays'}),
        dict(type='RGBLossMS', weight=0.1, img_size=[64, 64], no_ssim=False, ray_resize=[6, 10],
             input_dict={'ms_colors': 'ms_colors', 'ms_rays': 'ms_rays', 'gt_imgs': 'curr_imgs'})]))
    total, parts = loss_fn(dict(out, metas=metas, curr_imgs=imgs))
    assert set(parts) == {'SemCELossMS', 'RGBLossMS'}
    total.backward()
    last = f.density_net[-1]
    assert tuple(last.weight.shape) == (24, C)                               # sdf + 3 + 20 rows: the pad is not a parameter
    assert torch.isfinite(last.weight.grad).all() and torch.isfinite(last.bias.grad).all()
    assert (last.weight.grad.abs().amax(dim=1) > 0).all() and (last.bias.grad.abs() > 0).all()
    for r in rep:
        assert torch.isfinite(r.grad).all() and r.grad.abs().sum() > 0


def test_head_with_20_classes_renders_and_queries(hip):
    from selfocc_amd.occ import field_query
    os.environ['eval'] = 'true'
    try:
        head = _head(render_bkgd='white').eval()
        rep, metas, _ = _inputs(20)
        with torch.no_grad():
            head.prepare(rep, metas)
            out = head.render(metas, batch=90000)
            sem, acc = out['sem'][0], out['ms_accs'][0]
            assert sem.shape == (1, 2, 60, 20) and (acc > 0.05).sum() > 20
            assert (sem.sum(-1) - acc).abs().max() <= SUM_TOL
            res = head.forward_occ(rep, metas, aabb=AABB, resolution=0.4)
            assert res['logits'].shape == (32, 32, 7, 20)
            vol = head.model.field.volume
            q = field_query(vol.detached(), res['xyz'].reshape(-1, 3), want_sdf=True, want_logits=True, want_argmax=True)
            assert torch.equal(res['logits'].reshape(-1, 20), q['logits']) and torch.equal(res['sdf'].flatten(), q['sdf'])
            assert torch.equal(res['sem'].flatten(), q['argmax'].long())
    finally:
        os.environ['eval'] = 'false'


@pytest.mark.parametrize("color_dims", [23, 9])
def test_fused_and_op_by_op_field_routes_agree(hip, color_dims):
    """the fused MLP (inference kernel and the training Function) against the op-by-op route, per tensor within the largest
    (rel-L2, max / max) bound tests/test_field_sh_widths_gpu.py holds for it; the pad channels are exact zeros in all three"""
    from selfocc_amd.field import field_volume_supported, field_volume_train_supported
    from test_field_full_size_gpu import err
    from test_field_sh_widths_gpu import CEILING
    head = _head(color_dims).eval()
    f = head.model.field
    n_sem, F = color_dims - 3, stride(color_dims - 3)
    assert field_volume_supported(C, 2, 1 + color_dims, F) and field_volume_train_supported(C, 2, 1 + color_dims, F, torch.float32)
    rep, _, _ = _inputs(n_sem)
    vols = {}
    with torch.no_grad():
        vols['fused inference'] = f.pre_compute_density_color(rep)
        f.fused_volume = False
        vols['op by op'] = f.pre_compute_density_color(rep)
        f.fused_volume = True
    vols['fused training'] = f.pre_compute_density_color(rep).detached()
    ref = vols['op by op']
    for name, v in vols.items():
        assert tuple(v.feat.shape) == (32, 32, 4, F) and v.n_sem == n_sem
        assert v.feat[..., color_dims:].abs().max() == 0, name
        e_s, e_f = err(v.sdf, ref.sdf.double()), err(v.feat[..., :color_dims], ref.feat[..., :color_dims].double())
        print(f"\n[nsem field] color_dims={color_dims} {name}: sdf {e_s} feat {e_f}")
        assert e_s[0] <= CEILING['sdf'][0] and e_s[1] <= CEILING['sdf'][1], (name, e_s)
        assert e_f[0] <= CEILING['feat'][0] and e_f[1] <= CEILING['feat'][1], (name, e_f)
