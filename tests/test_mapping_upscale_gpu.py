"""GPU: the 'linear_upscale' grid mapping (NonLinearMapping, mappings.py:199-288) through the HIP kernels —
selfocc_meter2grid against the reference's own fixtures bit for bit, the canonical render (pixel grid and explicit rays),
the sample-parallel training forward and both backward scatters against the float64 torch port, field_query and its
backward against F.grid_sample, and two shipped configs switched to NeuSHead's default upscale mapping end to end."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_port as tp
from selfocc_amd import abi, render as rmod
from selfocc_amd.mapping import GridMeterMapping, meter2grid_device
from selfocc_amd.occ import field_query, field_query_autograd
from selfocc_amd.render import RaySet, RenderConfig, SDFVolume, render_rays, render_rays_autograd
from test_render_gpu import parity_report
from util import cell_margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D0 = torch.device("cuda:0")
geo = np.load(os.path.join(ROOT, "tests", "golden", "geometry.npz"))

# NeuSHead's default mapping_args (model/head/neus_head/neus_head.py): 321 x 321 x 31 lattice
HEAD_UPSCALE = dict(nonlinear_mode='linear_upscale', h_size=[128, 32], h_range=[51.2, 28.8], w_size=[128, 32],
                    w_range=[51.2, 28.8], d_size=[20, 10], d_range=[-4.0, 4.0, 12.0])
LINEAR = {
    'occ': dict(nonlinear_mode='linear', h_size=[128, 0], h_range=[40.0, 0], h_half=False, w_size=[128, 0],
                w_range=[40.0, 0], w_half=False, d_size=[24, 0], d_range=[-1.0, 5.4, 5.4]),
    'kitti': dict(nonlinear_mode='linear', h_size=[256, 0], h_range=[51.2, 0], h_half=True, w_size=[128, 0],
                  w_range=[25.6, 0], w_half=False, d_size=[32, 0], d_range=[-2.0, 4.4, 4.4]),
    'twoseg': dict(nonlinear_mode='linear', h_size=[128, 32], h_range=[51.2, 28.8], h_half=False,
                   w_size=[128, 32], w_range=[51.2, 28.8], w_half=False, d_size=[20, 10], d_range=[-4.0, 4.0, 12.0]),
}
AABB = (-80.0, -80.0, -4.0, 80.0, 80.0, 12.0)       # the whole upscale volume: inner 51.2 m + outer 28.8 m, z inner to 4 m


# ---------------------------------------------------------------------------------------------------------------------
# 1. the mapping itself
# ---------------------------------------------------------------------------------------------------------------------
def test_meter2grid_device_is_bit_exact_to_the_reference_fixtures(hip):
    m = GridMeterMapping(**HEAD_UPSCALE)
    xyz = torch.tensor(geo['upscale.xyz']).to(D0)
    assert torch.equal(meter2grid_device(m, xyz).cpu(), torch.tensor(geo['upscale.m2g']))
    assert torch.equal(meter2grid_device(m, xyz, True).cpu(), torch.tensor(geo['upscale.m2g_norm']))
    # the fixtures do reach the outer cells on every axis
    g = torch.tensor(geo['upscale.m2g'])
    assert ((g[:, 0] - 160).abs() > 128).any() and ((g[:, 1] - 160).abs() > 128).any() and (g[:, 2] > 20).any()
    for name, kw in LINEAR.items():
        lm = GridMeterMapping(**kw)
        xyz = torch.tensor(geo[f'{name}.xyz']).to(D0)
        assert torch.equal(meter2grid_device(lm, xyz).cpu(), torch.tensor(geo[f'{name}.m2g'])), name
        assert torch.equal(meter2grid_device(lm, xyz, True).cpu(), torch.tensor(geo[f'{name}.m2g_norm'])), name


def test_meter2grid_device_rejects_bad_parameters(hip):
    from selfocc_amd._lib import lib
    m = GridMeterMapping(**HEAD_UPSCALE).to_abi()
    m.uw.inc = -0.5
    xyz = torch.zeros(4, 3, device=D0)
    out = torch.empty_like(xyz)
    assert lib().selfocc_meter2grid(m, xyz.data_ptr(), 4, 0, out.data_ptr(), None) == -1
    assert lib().selfocc_last_error().decode().startswith("linear_upscale axis 1: increase unit must be > 0")
    m = GridMeterMapping(**HEAD_UPSCALE).to_abi()
    m.h.size1 = 0.0
    assert lib().selfocc_meter2grid(m, xyz.data_ptr(), 4, 0, out.data_ptr(), None) == -1
    assert "outer cells must be >= 1" in lib().selfocc_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------
# synthetic scene: ground, a cylindrical wall at 65 m (outer h / w cells) and a ceiling at 7 m (outer d cells)
# ---------------------------------------------------------------------------------------------------------------------
def _volume(m, n_rgb, n_sem, feat_dtype=torch.float32, seed=0):
    H, W, D = m.size_h, m.size_w, m.size_d
    g = torch.stack(torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64),
                                   torch.arange(D, dtype=torch.float64), indexing='ij'), -1)
    xyz = m.grid2meter(g)                                            # (H, W, D, 3) metres
    r = torch.linalg.norm(xyz[..., :2], dim=-1)
    sdf = torch.minimum(torch.minimum(xyz[..., 2] + 1.5, 65.0 - r), 7.0 - xyz[..., 2])
    gen = torch.Generator().manual_seed(seed)
    sdf = (sdf + 0.05 * torch.randn(sdf.shape, generator=gen, dtype=torch.float64)).float()
    dc = [sdf[None]]
    if n_rgb + n_sem:
        dc.append(torch.randn(n_rgb + n_sem, H, W, D, generator=gen))
    return SDFVolume.from_reference_layout(m, torch.cat(dc, 0)[None], n_rgb, n_sem, feat_dtype)


def _candidate_rays(n, seed):
    gen = torch.Generator().manual_seed(seed)
    az = torch.rand(n, generator=gen, dtype=torch.float64) * 2 * np.pi
    el = -0.25 + 0.75 * torch.rand(n, generator=gen, dtype=torch.float64)
    d = torch.stack([torch.cos(el) * torch.cos(az), torch.cos(el) * torch.sin(az), torch.sin(el)], -1)
    o = torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64) + 0.5 * torch.rand(n, 3, generator=gen, dtype=torch.float64) - 0.25
    return RaySet(origins=o.float().contiguous(), dirs=d.float().contiguous(), dir_norm=torch.ones(n))


def _off_faces(m, rays, cfg, margin):
    """explicit rays whose every sample lies >= margin voxels off every voxel face (float64)"""
    nears, fars = tp.aabb_collider(rays.origins.double(), rays.dirs.double(), cfg.aabb, cfg.near_plane)
    keep = cell_margin(m, rays, cfg, nears[:, 0], fars[:, 0]) >= margin
    idx = keep.nonzero()[:, 0]
    sub = RaySet(origins=rays.origins[idx].contiguous(), dirs=rays.dirs[idx].contiguous(), dir_norm=rays.dir_norm[idx].contiguous())
    return sub, idx


def _dev(rays):
    return RaySet(origins=rays.origins.to(D0), dirs=rays.dirs.to(D0), dir_norm=rays.dir_norm.to(D0))


def _coverage(m, rays, cfg):
    """every axis has samples in its outer cells"""
    nears, fars = tp.aabb_collider(rays.origins.double(), rays.dirs.double(), cfg.aabb, cfg.near_plane)
    b = torch.linspace(0, 1, cfg.n_samples + 1, dtype=torch.float64)
    t = (b[None] * fars + (1 - b[None]) * nears)[:, :-1]
    g = m.meter2grid(rays.origins.double()[:, None] + rays.dirs.double()[:, None] * t[..., None])
    assert ((g[..., 0] - 160).abs() > 128).any() and ((g[..., 1] - 160).abs() > 128).any() and (g[..., 2] > 20).any()


def _pixel_rays(n_cams=3, nx=24, ny=18, img=(90, 120), f=110.0, elev=0.15):
    """pinholes at the origin pitched up by `elev`: the lattice spans elevations ~ -0.24 .. 0.54 rad"""
    mats = []
    for i in range(n_cams):
        yaw = 2 * np.pi * i / n_cams + 0.3
        fwd = np.array([np.cos(elev) * np.cos(yaw), np.cos(elev) * np.sin(yaw), np.sin(elev)])
        right = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
        up = np.cross(right, fwd)
        cx, cy = img[1] / 2.0, img[0] / 2.0
        M = np.eye(4)
        M[:3, 0], M[:3, 1], M[:3, 2] = right / f, -up / f, fwd - cx / f * right + cy / f * up
        M[:3, 3] = [0.3, -0.2, 0.5]
        mats.append(M)
    return RaySet(img2lidar=torch.tensor(np.stack(mats), dtype=torch.float32), nx=nx, ny=ny, sx=img[1] / nx, sy=img[0] / ny)


# ---------------------------------------------------------------------------------------------------------------------
# 2. render forward (canonical route), pixel grid and explicit rays, C = 1 / 4 (f32, bf16) / 25
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rgb,n_sem,feat_dtype", [(0, 0, torch.float32), (3, 0, torch.float32), (3, 0, torch.bfloat16),
                                                    (3, 21, torch.float32)])
def test_render_forward_vs_float64_port(hip, n_rgb, n_sem, feat_dtype):
    from selfocc_amd import synthetic as sy
    m = GridMeterMapping(**HEAD_UPSCALE)
    vol = _volume(m, n_rgb, n_sem, feat_dtype)
    cfg = RenderConfig(aabb=AABB, n_samples=64, inv_s=20.0, sample_pos=abi.SAMPLE_AT_START)
    pix = _pixel_rays()
    ex_all = sy.explicit_rays(pix)
    ex, idx = _off_faces(m, ex_all, cfg, 1e-3)
    assert idx.numel() >= 300, idx.numel()
    _coverage(m, ex, cfg)
    dd = torch.float64
    ref = tp.render_port(m.mapping, vol.to_reference_layout().to(dd), n_rgb, n_sem, ex.origins.to(dd), ex.dirs.to(dd),
                         ex.dir_norm.to(dd), cfg)
    ref = {k: v.float() for k, v in ref.items()}
    assert (ref['acc'] > 0.05).float().mean() > 0.5          # most rays reach a surface
    v = vol.to(D0)
    n_ws = len(rmod._BRICK_WS)
    got = render_rays(v, _dev(ex), cfg)
    parity_report(got, ref, label=f"upscale explicit C={1 + n_rgb + n_sem} {feat_dtype}")
    gp = render_rays(v, RaySet(img2lidar=pix.img2lidar.to(D0), nx=pix.nx, ny=pix.ny, sx=pix.sx, sy=pix.sy), cfg)
    parity_report({k: t[idx.to(D0)] for k, t in gp.items()}, ref, label=f"upscale pixel grid C={1 + n_rgb + n_sem} {feat_dtype}")
    gt = render_rays(v, _dev(ex), cfg, per_sample=True)      # the sample-parallel kernel of the same row
    parity_report({k: gt[k] for k in got}, ref, label=f"upscale per-sample launch C={1 + n_rgb + n_sem} {feat_dtype}")
    assert len(rmod._BRICK_WS) == n_ws                       # no brick re-pack for the upscale route


# ---------------------------------------------------------------------------------------------------------------------
# 3. training forward (per-sample outputs) and backward, both scatters
# ---------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("scatter", ["atomic", "binned"])
@pytest.mark.parametrize("n_rgb,n_sem,S,sample_pos", [(0, 0, 48, 0), (3, 0, 100, 1), (3, 21, 48, 0)])
def test_training_forward_and_backward_vs_float64_autograd(hip, n_rgb, n_sem, S, sample_pos, scatter):
    m = GridMeterMapping(**HEAD_UPSCALE)
    vol = _volume(m, n_rgb, n_sem, seed=1)
    cfg = RenderConfig(aabb=AABB, n_samples=S, inv_s=12.0, sample_pos=sample_pos,
                       bkgd_mode=abi.BKGD_PER_RAY if n_rgb else abi.BKGD_NONE)
    cfg.bwd_scatter = scatter
    # the port's slope is a forward difference over 1e-3 m (<= 0.0025 voxel): keep every sample 4e-3 voxel off any face
    ex, _ = _off_faces(m, _candidate_rays(6000, seed=S), cfg, 4e-3)
    N = ex.origins.shape[0]
    assert N >= 150, N
    _coverage(m, ex, cfg)
    g = torch.Generator().manual_seed(3)
    bk = torch.rand(N, 3, generator=g) if n_rgb else None
    G = dict(depth=torch.randn(N, generator=g), acc=torch.randn(N, generator=g), weights=torch.randn(N, S, generator=g),
             sdf=0.1 * torch.randn(N, S, generator=g), grad=0.1 * torch.randn(N, S, 3, generator=g))
    if n_rgb:
        G['rgb'] = torch.randn(N, 3, generator=g)
    if n_sem:
        G['sem'] = torch.randn(N, n_sem, generator=g)

    dd = torch.float64
    vol64 = vol.to_reference_layout()[0].to(dd).requires_grad_(True)
    inv_s64 = torch.tensor(cfg.inv_s, dtype=dd, requires_grad=True)
    ref = tp.render_port_differentiable(m.mapping, vol64, n_rgb, n_sem, ex.origins.to(dd), ex.dirs.to(dd),
                                        ex.dir_norm.to(dd), cfg, inv_s64, None, None if bk is None else bk.to(dd))
    sum((ref[k] * G[k].to(dd)).sum() for k in G).backward()
    ref_gsdf = vol64.grad[0]
    ref_gfeat = vol64.grad[1:].permute(1, 2, 3, 0) if n_rgb + n_sem else None

    v = vol.to(D0)
    sdf_p = v.sdf.clone().requires_grad_(True)
    feat_p = None if v.feat is None else v.feat.clone().requires_grad_(True)
    inv_s = torch.tensor([cfg.inv_s], device=D0, requires_grad=True)
    out = render_rays_autograd(SDFVolume(m, sdf_p, feat_p, n_rgb, n_sem), inv_s, _dev(ex), cfg, want_grad_samples=True,
                               bkgd_rays=None if bk is None else bk.to(D0))
    for k in G:
        assert torch.allclose(out[k].detach().cpu().double(), ref[k].detach(), rtol=2e-3, atol=2e-4), k
    sum((out[k] * G[k].to(D0)).sum() for k in G).backward()
    e_sdf = _rel_l2(sdf_p.grad.cpu().double(), ref_gsdf)
    assert e_sdf < 2e-3, f"d/d sdf_vol rel L2 {e_sdf:.3e}"
    assert (sdf_p.grad.cpu().double() - ref_gsdf).abs().max() < 2e-2 * ref_gsdf.abs().max()
    if ref_gfeat is not None:
        got = feat_p.grad.cpu().double()[..., :n_rgb + n_sem]
        e_f = _rel_l2(got, ref_gfeat)
        assert e_f < 2e-3, f"d/d feat_vol rel L2 {e_f:.3e}"
    e_s = abs(inv_s.grad.item() - inv_s64.grad.item()) / (abs(inv_s64.grad.item()) + 1e-12)
    assert e_s < 5e-2, f"d/d inv_s rel {e_s:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# 4. field_query / field_query_bwd against F.grid_sample on meter2grid(xyz, True) * 2 - 1
# ---------------------------------------------------------------------------------------------------------------------
def test_field_query_and_backward_vs_grid_sample(hip):
    m = GridMeterMapping(**HEAD_UPSCALE)
    n_sem = 17
    vol = _volume(m, 3, n_sem, seed=2)
    gen = torch.Generator().manual_seed(4)
    n = 50000
    xyz = (torch.rand(n, 3, generator=gen) * torch.tensor([170.0, 170.0, 18.0]) - torch.tensor([85.0, 85.0, 5.0])).contiguous()
    dc = vol.to_reference_layout()                                # (1, C, H, W, D)
    # meter2grid in the reference's float32 order: the device form, pinned bit for bit to the reference's fixtures above
    # (the host mirror NonLinearMapping.meter2grid associates one sum differently and agrees to ~1 ulp only)
    grid = (meter2grid_device(m, xyz.to(D0), True).cpu() * 2 - 1).reshape(1, -1, 1, 1, 3)[..., [2, 1, 0]]
    dc_p = dc.clone().requires_grad_(True)
    ref = F.grid_sample(dc_p, grid, mode='bilinear', align_corners=True).reshape(dc.shape[1], n).T   # (n, C)
    v = vol.to(D0)
    q = field_query(v, xyz.to(D0), want_logits=True)
    assert torch.equal(q['sdf'].cpu(), ref[:, 0].detach())
    assert torch.equal(q['logits'].cpu(), ref[:, 4:].detach())
    gs, gl = torch.randn(n, generator=gen), torch.randn(n, n_sem, generator=gen)
    ((ref[:, 0] * gs).sum() + (ref[:, 4:] * gl).sum()).backward()
    sdf_p = v.sdf.clone().requires_grad_(True)
    feat_p = v.feat.clone().requires_grad_(True)
    qa = field_query_autograd(SDFVolume(m, sdf_p, feat_p, 3, n_sem), xyz.to(D0), want_logits=True)
    ((qa['sdf'] * gs.to(D0)).sum() + (qa['logits'] * gl.to(D0)).sum()).backward()
    assert _rel_l2(sdf_p.grad.cpu().double(), dc_p.grad[0, 0].double()) < 1e-5
    assert _rel_l2(feat_p.grad.cpu().double()[..., 3:], dc_p.grad[0, 4:].permute(1, 2, 3, 0).double()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 5. shipped configs switched to NeuSHead's default upscale mapping: one training iteration + the evaluation entry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['nuscenes_depth', 'nuscenes_occ'])
def test_shipped_config_with_upscale_mapping_trains_and_evaluates(hip, name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import hotpath_common as hc
    from test_shipped_configs_gpu import no_sync
    torch.manual_seed(0)
    np.random.seed(0)
    os.environ['eval'] = 'false'
    cfg = hc.upscale_variant(hc.shipped(name))
    mods = hc.build(cfg, D0, want_loss=True)
    lifter, encoder, head, loss_fn = mods
    assert cfg['model']['head']['mapping_args'] == dict(HEAD_UPSCALE, h_half=False, w_half=False)
    assert head.model.field.mapping.nonlinear_mode == 'linear_upscale'
    assert (head.model.field.size_h, head.model.field.size_w, head.model.field.size_d) == (321, 321, 31)
    for mod in (lifter, encoder, head):
        mod.train()
    g = torch.Generator(device='cpu').manual_seed(3)
    with torch.no_grad():
        for mod in (lifter, encoder, head):
            for p in mod.parameters():
                if float(p.abs().max()) == 0.0:
                    p.copy_((0.02 * torch.randn(p.shape, generator=g)).to(p.device))
    params = [(f'{tag}.{n}', p) for tag, mod in (('lifter', lifter), ('encoder', encoder), ('head', head))
              for n, p in mod.named_parameters()]
    hc.train_iteration(mods, cfg, hc.frame_inputs(cfg, name, D0, seed=0), global_iter=0)
    for _, p in params:
        p.grad = None
    new = hc.frame_inputs(cfg, name, D0, seed=1)
    with no_sync():
        total, parts, out = hc.train_iteration(mods, cfg, new, global_iter=1)
    assert torch.isfinite(total).all() and float(total) != 0.0
    for k, v in parts.items():
        assert np.isfinite(float(v)), (name, k, float(v))
    bad = [n for n, p in params if p.requires_grad and (p.grad is None or not torch.isfinite(p.grad).all()
                                                       or float(p.grad.abs().max()) == 0.0)]
    assert not bad, (name, bad[:8], len(bad))
    del mods, lifter, encoder, head, loss_fn, params, out, total, parts, new
    torch.cuda.empty_cache()

    os.environ['eval'] = 'true'
    try:
        ecfg = hc.upscale_variant(hc.shipped_for_eval(name))
        emods = hc.build(ecfg, D0)
        for mod in emods[:3]:
            mod.eval()
        state = {}
        with torch.no_grad():
            hc.eval_entry(emods, ecfg, name, hc.frame_inputs(ecfg, name, D0, seed=2, want_images=False), state)
            new = hc.frame_inputs(ecfg, name, D0, seed=3, want_images=False)
            with no_sync():
                res = hc.eval_entry(emods, ecfg, name, new, state)
        if hc.SHIPPED[name]['eval'] == 'render':
            d = res['ms_depths'][0]
            assert torch.isfinite(d).all() and float(d.max()) > 0
            assert torch.isfinite(res['ms_max_depths'][0]).all() and torch.isfinite(res['ms_accs'][0]).all()
        else:
            assert res['sdf'].shape == (400, 400, 40) and torch.isfinite(res['sdf']).all()    # roi_aabb at 0.4 m
            assert res['occ'].shape == (200, 200, 16) and torch.isfinite(res['logits']).all()
            miou, iou = state['miou']._after_epoch()
            assert np.isfinite(miou) and np.isfinite(iou)
    finally:
        os.environ['eval'] = 'false'
