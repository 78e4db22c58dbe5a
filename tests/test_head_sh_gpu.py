"""GPU: NeuSHead with view-dependent colour (color_dims = 27, sh_deg = 2) end to end — training forward + backward without a
host synchronisation, ``ms_colors`` against the float64 composition (tests/sh_compose.py) evaluated on the head's own volume,
the gradient of the 27 colour rows of the last density_net Linear against float64 autograd through field MLP + composition,
and the eval ``render()``.  Once on a small linear mapping, once on NeuSHead's default 'linear_upscale' mapping_args."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from selfocc_amd import abi, sh, synthetic as sy
from selfocc_amd.registry import MODELS
from selfocc_amd.render import RaySet, RenderConfig
import selfocc_amd.model  # noqa: F401
from sh_compose import compose64
import test_mapping_upscale_gpu as up

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
C = 96            # embed_dims the fused field MLP is built for: the 28-wide coefficient volume comes from FieldVolumeFunction


class no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *a):
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def _head(kind, sh_act='relu'):
    kw = dict(type='NeuSHead', resolution=0.4, num_samples=32, num_samples_importance=0, num_up_sample_steps=0, beta_init=0.25,
              use_numerical_gradients=False, ray_sample_mode='fixed', trans_kw='img2lidar', render_bkgd='white', embed_dims=C,
              color_dims=27, density_layers=2, sh_deg=2, sh_act=sh_act, two_split=False, tpv=True)
    if kind == 'small':
        kw.update(roi_aabb=list(sy.CONFIGS["cfg1"]["aabb"]), mapping_args=sy.CONFIGS["cfg1"]["mapping"], ray_number=[6, 10],
                  ray_img_size=[64, 64])
        cams = sy.make_cameras("cfg1", 0).repeat(2, 1, 1).clone()
        cams[1:, :3, 3] += torch.tensor([0.5, -0.3, 0.0])
    else:       # NeuSHead's own default mapping_args ('linear_upscale', 321 x 321 x 31)
        kw.update(roi_aabb=list(up.AABB), ray_number=[18, 24], ray_img_size=[90, 120], num_samples=64)
        cams = up._pixel_rays(n_cams=2).img2lidar
    torch.manual_seed(0)
    head = MODELS.build(kw).to(D0)
    f = head.model.field
    assert (f.sh_deg, f.sh_act, f.n_rgb, f.n_sem) == (2, sh_act, 3, 0)
    if kind != 'small':
        assert f.mapping.nonlinear_mode == 'linear_upscale' and (f.size_h, f.size_w, f.size_d) == (321, 321, 31)
    H, W, Z = f.size_h, f.size_w, f.size_d
    g = torch.Generator().manual_seed(1)
    scale = 1.0 if kind == 'small' else 0.3
    rep = [(scale * torch.randn(1, n, C, generator=g)).to(D0).requires_grad_(True) for n in (H * W, Z * H, W * Z)]
    with torch.no_grad():
        # surfaces inside the box: rescale the SDF row of the last Linear so that the field has mean +0.5 m and deviation 1 m
        # (zero crossings along most rays); with the initial weights every ray would accumulate < 0.01 — a test of the background
        s0 = f.pre_compute_density_color(rep).sdf
        mean, std = s0.mean(), s0.std()
        last = f.density_net[-1]
        last.weight[0] /= std
        last.bias[0] = (last.bias[0] - mean) / std + 0.5
    metas = [dict(img2lidar=cams.numpy(), img_shape=tuple(kw['ray_img_size']))]
    return head, rep, metas, cams


def _lattice(head, cams):
    s = head.ray_sampler
    ny, nx = s.ray_resize
    lat = s.lattice()
    return RaySet(img2lidar=cams, nx=nx, ny=ny, sx=float(np.float32(lat[0])), sy=float(np.float32(lat[1])),
                  ox=float(np.float32(lat[2])), oy=float(np.float32(lat[3])))


@pytest.mark.parametrize("kind,sh_act", [('small', 'relu'), ('small', 'sigmoid'), ('default_upscale', 'relu')])
def test_head_with_sh_colour_trains_and_renders(hip, kind, sh_act):
    os.environ['eval'] = 'false'
    head, rep, metas, cams = _head(kind, sh_act)
    head.train()
    f = head.model.field
    n_cams = cams.shape[0]
    pix = _lattice(head, cams)
    ex = sy.explicit_rays(pix)
    N, S = ex.n_rays, head.num_samples
    Gc = torch.randn(1, n_cams, N // n_cams, 3, generator=torch.Generator().manual_seed(2)).to(D0)

    def step(seed):
        for p in list(head.parameters()) + rep:
            p.grad = None
        torch.manual_seed(seed)
        out = head(rep, metas, global_iter=0)
        ((out['ms_colors'][0] * Gc).sum() + out['ms_depths'][0].mean()).backward()
        return out
    step(5)                                # warm-up: lazy workspaces, the cached lattice
    with no_sync():
        out = step(6)
    torch.manual_seed(6)
    t_rand = torch.rand(N, device=D0).cpu()            # the head's single jitter draw (its only draw: constant background)
    assert out['ms_colors'][0].shape == (1, n_cams, N // n_cams, 3)
    assert tuple(f.volume.feat.shape) == (f.size_h, f.size_w, f.size_d, 28) and f.volume.sh_deg == 2
    assert f.volume.feat[..., 27].abs().max().item() == 0.0
    wg = f.density_net[-1].weight.grad
    assert wg.shape == (28, C) and torch.isfinite(wg).all()
    assert (wg[1:28].abs().amax(dim=1) > 0).all()                     # every one of the 27 colour rows
    for p in list(head.parameters()) + rep:
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert f.variance.grad.abs().item() > 0

    # ---- ms_colors == the float64 composition on the head's own volume ------------------------------------------------------
    cfg = head._render_cfg(True)
    assert cfg.jitter_mode == abi.JITTER_SINGLE and cfg.bkgd_mode == abi.BKGD_CONST and not cfg.clamp_rgb
    vol = f.volume
    inv_s = f.inv_s().detach().double().cpu()[0]
    keep = torch.arange(N)
    if kind != 'small':
        # the float64 port is a reference only for rays whose samples keep off the voxel faces (tests/test_render_sh_gpu.py)
        from oracle import torch_port as tp
        nears, fars = tp.aabb_collider(ex.origins.double(), ex.dirs.double(), cfg.aabb, cfg.near_plane)
        b = torch.linspace(0, 1, S + 1, dtype=torch.float64)[None]
        ctr = (b[:, 1:] + b[:, :-1]) / 2
        lo, hi = torch.cat([b[:, :1], ctr], -1), torch.cat([ctr, b[:, -1:]], -1)
        t = ((lo + (hi - lo) * t_rand.double()[:, None]) * fars + (1 - (lo + (hi - lo) * t_rand.double()[:, None])) * nears)[:, :-1]
        gc = vol.mapping.meter2grid(ex.origins.double()[:, None] + ex.dirs.double()[:, None] * t[..., None])
        fr = gc - torch.floor(gc)
        keep = (torch.minimum(fr, 1 - fr).amin(dim=(1, 2)) > 1e-3).nonzero()[:, 0]
        assert keep.numel() > N // 2
    sub = RaySet(origins=ex.origins[keep].contiguous(), dirs=ex.dirs[keep].contiguous(), dir_norm=ex.dir_norm[keep].contiguous())
    ref = compose64(vol.mapping, vol.sdf.detach().double().cpu(), vol.feat.detach().double().cpu(), 2, sh_act, sub, cfg, inv_s,
                    t_rand[keep].contiguous())
    got = out['ms_colors'][0].detach().reshape(-1, 3).cpu().double()[keep]
    d = (got - ref['rgb']).abs().max().item()
    print(f"\n[head sh {kind} {sh_act}] train max |ms_colors - f64| = {d:.3e}; rays with acc > 0.05: {(ref['acc'] > 0.05).sum().item()}")
    assert d <= 1e-4
    assert (ref['acc'] > 0.05).sum() > 10

    if kind == 'small':
        # ---- the 27 colour rows of the last Linear: float64 autograd through field MLP + composition ------------------------
        dd = torch.float64
        H, W, Z = f.size_h, f.size_w, f.size_d
        lin = [m for m in f.density_net if isinstance(m, torch.nn.Linear)]
        w1, b1, w2, b2 = (t.detach().cpu().to(dd).requires_grad_(True) for t in (lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias))
        hw, zh, wz = (t.detach().cpu().to(dd) for t in rep)
        x = hw.reshape(H, W, 1, C) + zh.reshape(Z, H, 1, C).permute(1, 2, 0, 3) + wz.reshape(W, Z, 1, C).permute(2, 0, 1, 3)
        o = Fn.linear(Fn.softplus(Fn.linear(Fn.softplus(x), w1, b1)), w2, b2)
        feat64 = torch.cat([o[..., 1:], o.new_zeros(H, W, Z, 1)], -1)
        var64 = f.variance.detach().cpu().to(dd).requires_grad_(True)
        ref2 = compose64(vol.mapping, o[..., 0], feat64, 2, sh_act, ex, cfg, torch.exp(var64 * 10.0).clip(1e-6, 1e6)[0], t_rand)
        depth = ref2['depth'].reshape(1, n_cams, -1)
        ((ref2['rgb'].reshape(1, n_cams, -1, 3) * Gc.cpu().to(dd)).sum() + depth.mean()).backward()
        e = ((wg[1:28].cpu().double() - w2.grad[1:28]).norm() / w2.grad[1:28].norm()).item()
        eb = ((lin[1].bias.grad[1:28].cpu().double() - b2.grad[1:28]).norm() / b2.grad[1:28].norm()).item()
        print(f"[head sh {kind} {sh_act}] colour rows of d L / d W2: rel-L2 {e:.3e}, d L / d b2: {eb:.3e}")
        assert e < 2e-3 and eb < 2e-3

    # ---- eval: render() returns clamped ms_colors by the same rule ----------------------------------------------------------
    os.environ['eval'] = 'true'
    try:
        head.eval()
        with torch.no_grad():
            head.prepare(rep, metas)
            with no_sync():
                r = head.render(metas)
        cfg_e = head._render_cfg(False)
        assert cfg_e.clamp_rgb and cfg_e.jitter_mode == abi.JITTER_NONE
        vol = f.volume
        pe = _lattice(type('S', (), dict(ray_sampler=head.ray_sampler_eval))(), cams)
        exe = sy.explicit_rays(pe)
        if kind != 'small':
            exe, keep = up._off_faces(vol.mapping, exe, cfg_e, 1e-3)
        else:
            keep = torch.arange(exe.n_rays)
        ref = compose64(vol.mapping, vol.sdf.double().cpu(), vol.feat.double().cpu(), 2, sh_act, exe, cfg_e, inv_s)
        got = r['ms_colors'][0].reshape(-1, 3).cpu().double()[keep]
        d = (got - ref['rgb']).abs().max().item()
        print(f"[head sh {kind} {sh_act}] eval max |ms_colors - f64| = {d:.3e}")
        assert d <= 1e-4 and got.min() >= 0.0 and got.max() <= 1.0
    finally:
        os.environ['eval'] = 'false'
