"""GPU: view-dependent colour (spherical harmonics of degree 1 / 2, relu / sigmoid) in the render forward, the training
(per-sample) forward and the render backward.

References, none of which the feature touches: the C oracle (degree-0 colour) through the BUNDLE IDENTITY — for rays that share
one direction d, a spherical-harmonics render of coefficients F equals the degree-0 render of the reduced 3-channel volume
V_c = sum_k Y_k(d) F[c, k] / C0 — and a float64 composition of the torch port's parts (tests/sh_compose.py)."""
import json
import os

import pytest
import torch

import oracle
from selfocc_amd import abi, sh, synthetic as sy
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import render_rays, render_rays_autograd, RaySet, RenderConfig, SDFVolume
from sh_compose import compose64
from test_render_gpu import _cmp, parity_report
import test_mapping_upscale_gpu as up

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
C0 = 0.28209479177387814
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The 'linear_upscale' variant.  cfg1's mapping has half axes (the box starts at 0), which NonLinearMapping does not have,
# so the upscale cases run on the scene of tests/test_mapping_upscale_gpu.py (NeuSHead's default mapping, 321 x 321 x 31: ground,
# a wall in the outer h / w cells, a ceiling in the outer d cells), with its rays and its rule for them: the float64 port takes
# d grid / d metre as a forward difference over 1e-3 m, so it is only a reference for rays whose samples keep off voxel faces.


def _dev_rays(ex):
    return RaySet(origins=ex.origins.to(D0), dirs=ex.dirs.to(D0), dir_norm=None if ex.dir_norm is None else ex.dir_norm.to(D0))


def _rel_l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _volume(deg, act, seed=3, noise=0.05):
    return sy.make_volume("cfg1", n_rgb=3, sh_deg=deg, sh_act=act, seed=seed, noise=noise)


def _upscale_volume(deg, act, seed=0):
    m = GridMeterMapping(**up.HEAD_UPSCALE)
    sdf = up._volume(m, 0, 0, seed=seed).sdf
    feat = torch.zeros(*sdf.shape, sh.feat_stride(deg))
    feat[..., :sh.n_coef(deg)] = torch.randn(*sdf.shape, sh.n_coef(deg), generator=torch.Generator().manual_seed(seed + 1))
    return SDFVolume(m, sdf, feat, 3, 0, deg, act)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("deg,sample_pos,jitter", [(1, 0, abi.JITTER_NONE), (1, 1, abi.JITTER_NONE), (2, 0, abi.JITTER_NONE),
                                                   (2, 1, abi.JITTER_NONE), (2, 0, abi.JITTER_SINGLE)])
def test_sh_forward_vs_c_oracle_by_the_bundle_identity(hip, deg, sample_pos, jitter, exact):
    """8 bundles of 64 explicit rays, one direction per bundle, all 512 rendered by ONE spherical-harmonics launch; each
    bundle against the C oracle on its reduced volume.  The oracle through this identity is within 1.6e-6 / 2.7e-6 (degree 1 / 2)
    of a float64 composition of the same render (measured on the CPU), so 1e-4 leaves ~40 x over the reference's own rounding."""
    vol = _volume(deg, 'relu')
    nb = sh.n_basis(deg)
    H, W, D = vol.sdf.shape
    G, per = 8, 64
    g = torch.Generator().manual_seed(1)
    dirs, origins = [], []
    for _ in range(G):
        d = torch.randn(3, generator=g)
        d[2] *= 0.2
        dirs.append((d / d.norm())[None].expand(per, 3))
        origins.append(torch.tensor([6.4, 6.4, 0.5]) + (torch.rand(per, 3, generator=g) - 0.5) * torch.tensor([8.0, 8.0, 1.0]))
    ex = RaySet(origins=torch.cat(origins).contiguous(), dirs=torch.cat(dirs).contiguous(), dir_norm=torch.ones(G * per))
    cfg = sy.make_render_config("cfg1", inv_s=20.0, sample_pos=sample_pos, jitter_mode=jitter, bkgd_mode=abi.BKGD_CONST,
                                bkgd=(1.0, 0.5, 0.25), clamp_rgb=True, exact=exact)
    t_rand = torch.rand(G * per, generator=g) if jitter != abi.JITTER_NONE else None
    got = render_rays(vol.to(D0), _dev_rays(ex), cfg, t_rand=None if t_rand is None else t_rand.to(D0))
    torch.cuda.synchronize()
    n_hit = 0
    coef = vol.feat[..., :3 * nb].reshape(H, W, D, 3, nb)
    for b in range(G):
        sl = slice(b * per, (b + 1) * per)
        basis = sh.sh_basis(deg, ex.dirs[b * per])
        feat = torch.zeros(H, W, D, 4)
        feat[..., :3] = (coef * basis).sum(-1) / C0
        sub = RaySet(origins=ex.origins[sl].contiguous(), dirs=ex.dirs[sl].contiguous(), dir_norm=ex.dir_norm[sl].contiguous())
        ref = oracle.render_fwd(SDFVolume(vol.mapping, vol.sdf, feat.contiguous(), 3, 0), sub, cfg,
                                t_rand=None if t_rand is None else t_rand[sl].contiguous())
        mine = {k: v[sl] for k, v in got.items()}
        n_hit += int((ref['acc'] > 0.05).sum())
        if exact:
            d = (mine['rgb'].cpu() - ref['rgb']).abs()
            print(f"\n[sh bundle {b} deg {deg}] max |rgb - oracle| = {d.max().item():.3e}")
            assert (d <= 1e-4 + 1e-4 * ref['rgb'].abs()).all(), d.max().item()          # the strict rgb rule, every ray
            _cmp(mine, ref, keys=['depth', 'acc', 'nears', 'fars', 'max_depth'])
        else:
            parity_report(mine, ref, label=f"sh bundle {b} deg {deg}")
    assert n_hit > 128          # not a test of the background


@pytest.mark.parametrize("deg,act", [(0, 'sigmoid'), (1, 'relu'), (1, 'sigmoid'), (2, 'relu'), (2, 'sigmoid')])
def test_sh_forward_pixel_grid_vs_float64_composition(hip, deg, act):
    """the cfg1 lattice (1 000 rays, every ray its own direction, generated in-kernel) against the float64 composition"""
    mapping = 'linear'
    vol = _volume(deg, act)
    rays = sy.make_rays("cfg1", seed=3)
    ex = sy.explicit_rays(rays)
    cfg = sy.make_render_config("cfg1", inv_s=20.0, bkgd_mode=abi.BKGD_CONST, bkgd=(1.0, 0.5, 0.25), clamp_rgb=True, exact=True)
    ref = compose64(vol.mapping, vol.sdf.double(), vol.feat.double(), deg, act, ex, cfg, torch.tensor(cfg.inv_s, dtype=torch.float64))
    got = render_rays(vol.to(D0), RaySet(img2lidar=rays.img2lidar.to(D0), nx=rays.nx, ny=rays.ny, sx=rays.sx, sy=rays.sy), cfg)
    got_ex = render_rays(vol.to(D0), _dev_rays(ex), cfg)
    torch.cuda.synchronize()
    assert (ref['acc'] > 0.05).sum() > 100
    for name, o in (("pixel grid", got), ("explicit", got_ex)):
        d = (o['rgb'].cpu().double() - ref['rgb']).abs()
        print(f"\n[sh {name} deg {deg} {act} {mapping}] max |rgb - f64| = {d.max().item():.3e}")
        assert d.max().item() <= 1e-4, (name, d.max().item())
        assert torch.allclose(o['acc'].cpu().double(), ref['acc'], rtol=1e-4, atol=1e-5)
    # default flags: the same launch (spherical-harmonics launches always march canonically)
    cfg.exact = False
    fast = render_rays(vol.to(D0), RaySet(img2lidar=rays.img2lidar.to(D0), nx=rays.nx, ny=rays.ny, sx=rays.sx, sy=rays.sy), cfg)
    assert (fast['rgb'].cpu().double() - ref['rgb']).abs().max().item() <= 1e-4


@pytest.mark.parametrize("deg,act", [(0, 'sigmoid'), (1, 'relu'), (2, 'relu'), (2, 'sigmoid')])
def test_sh_forward_under_the_upscale_mapping_vs_float64_composition(hip, deg, act):
    """eval forward (pixel grid and explicit) and training forward under 'linear_upscale', rays off the voxel faces"""
    vol = _upscale_volume(deg, act)
    m = vol.mapping
    cfg = RenderConfig(aabb=up.AABB, n_samples=64, inv_s=20.0, sample_pos=abi.SAMPLE_AT_START, bkgd_mode=abi.BKGD_CONST,
                       bkgd=(1.0, 0.5, 0.25), clamp_rgb=True, exact=True)
    pix = up._pixel_rays()
    ex, idx = up._off_faces(m, sy.explicit_rays(pix), cfg, 1e-3)
    assert idx.numel() >= 300, idx.numel()
    up._coverage(m, ex, cfg)
    ref = compose64(m, vol.sdf.double(), vol.feat.double(), deg, act, ex, cfg, torch.tensor(cfg.inv_s, dtype=torch.float64))
    assert (ref['acc'] > 0.05).float().mean() > 0.5
    v = vol.to(D0)
    rg = RaySet(img2lidar=pix.img2lidar.to(D0), nx=pix.nx, ny=pix.ny, sx=pix.sx, sy=pix.sy)
    gp = render_rays(v, rg, cfg)
    ge = render_rays(v, _dev_rays(ex), cfg)
    gt = render_rays(v, rg, cfg, per_sample=True, want_grad_samples=True)
    plain = render_rays(SDFVolume(m, v.sdf), rg, cfg, per_sample=True, want_grad_samples=True)
    torch.cuda.synchronize()
    for name, rgb in (("pixel grid", gp['rgb'][idx.to(D0)]), ("explicit", ge['rgb']), ("training", gt['rgb'][idx.to(D0)])):
        d = (rgb.cpu().double() - ref['rgb']).abs()
        print(f"\n[sh upscale {name} deg {deg} {act}] max |rgb - f64| = {d.max().item():.3e}")
        assert d.max().item() <= 1e-4, (name, d.max().item())
    for k in ('weights', 'ts', 'deltas', 'sdf', 'grad', 'depth', 'acc'):
        assert torch.equal(gt[k], plain[k]), k


@pytest.mark.parametrize("deg,act,S,jitter", [(1, 'relu', 32, abi.JITTER_SINGLE), (2, 'relu', 100, abi.JITTER_NONE),
                                              (2, 'sigmoid', 256, abi.JITTER_PER_BIN), (0, 'sigmoid', 32, abi.JITTER_NONE)])
def test_sh_training_forward(hip, deg, act, S, jitter):
    mapping = 'linear'
    """per_sample=True (the sample-parallel kernel, 1 / 2 / 4 waves per ray): per-ray rgb against the float64 composition;
    weights / ts / deltas / sdf / grad BITWISE equal to the SDF-only launch of the same rays — colour must not perturb them"""
    vol = _volume(deg, act)
    rays = sy.make_rays("cfg1", seed=3)
    ex = sy.explicit_rays(rays)
    cfg = sy.make_render_config("cfg1", inv_s=20.0, jitter_mode=jitter, bkgd_mode=abi.BKGD_PER_RAY)
    cfg.n_samples = S
    N = ex.n_rays
    g = torch.Generator().manual_seed(5)
    t_rand = None if jitter == abi.JITTER_NONE else torch.rand(*((N,) if jitter == abi.JITTER_SINGLE else (N, S + 1)), generator=g)
    bk = torch.rand(N, 3, generator=g)
    ref = compose64(vol.mapping, vol.sdf.double(), vol.feat.double(), deg, act, ex, cfg, torch.tensor(cfg.inv_s, dtype=torch.float64),
                    t_rand, bk)
    tr = None if t_rand is None else t_rand.to(D0)
    rg = RaySet(img2lidar=rays.img2lidar.to(D0), nx=rays.nx, ny=rays.ny, sx=rays.sx, sy=rays.sy)
    got = render_rays(vol.to(D0), rg, cfg, per_sample=True, want_grad_samples=True, t_rand=tr, bkgd_rays=bk.to(D0))
    cfg0 = sy.make_render_config("cfg1", inv_s=20.0, jitter_mode=jitter)
    cfg0.n_samples = S
    plain = render_rays(SDFVolume(vol.mapping, vol.sdf.to(D0)), rg, cfg0, per_sample=True, want_grad_samples=True, t_rand=tr)
    torch.cuda.synchronize()
    d = (got['rgb'].cpu().double() - ref['rgb']).abs()
    print(f"\n[sh train deg {deg} {act} S {S} {mapping}] max |rgb - f64| = {d.max().item():.3e}")
    assert d.max().item() <= 1e-4
    for k in ('weights', 'ts', 'deltas', 'sdf', 'grad', 'depth', 'acc', 'max_depth', 'nears', 'fars'):
        assert torch.equal(got[k], plain[k]), k


def _backward_case(deg, act, jitter, sample_pos, S, scatter, upscale=False, zero=False):
    if upscale:
        vol = _upscale_volume(deg, act, seed=1)
        cfg = RenderConfig(aabb=up.AABB, n_samples=S, inv_s=12.0, sample_pos=sample_pos, jitter_mode=jitter, bkgd_mode=abi.BKGD_PER_RAY)
        cfg.bwd_scatter = scatter
        # the port's slope is a forward difference over 1e-3 m (<= 0.0025 voxel): keep every sample 4e-3 voxel off any face
        ex, _ = up._off_faces(vol.mapping, up._candidate_rays(6000, seed=S), cfg, 4e-3)
        assert ex.n_rays >= 150
        up._coverage(vol.mapping, ex, cfg)
    else:
        vol = _volume(deg, act, seed=11, noise=0.02)
        ex = sy.explicit_rays(sy.make_rays("cfg1", seed=11))
        cfg = sy.make_render_config("cfg1", inv_s=12.0, sample_pos=sample_pos, jitter_mode=jitter, bkgd_mode=abi.BKGD_PER_RAY)
        cfg.n_samples = S
        cfg.bwd_scatter = scatter
    N = ex.n_rays
    g = torch.Generator().manual_seed(3)
    t_rand = None if jitter == abi.JITTER_NONE else torch.rand(*((N,) if jitter == abi.JITTER_SINGLE else (N, S + 1)), generator=g)
    bk = torch.rand(N, 3, generator=g)
    G = dict(depth=torch.randn(N, generator=g), acc=torch.randn(N, generator=g), weights=torch.randn(N, S, generator=g),
             sdf=0.1 * torch.randn(N, S, generator=g), grad=0.1 * torch.randn(N, S, 3, generator=g), rgb=torch.randn(N, 3, generator=g))
    if zero:
        G = {k: torch.zeros_like(v) for k, v in G.items()}
    v = vol.to(D0)
    sdf_p, feat_p = v.sdf.clone().requires_grad_(True), v.feat.clone().requires_grad_(True)
    inv_s = torch.tensor([cfg.inv_s], device=D0, requires_grad=True)
    out = render_rays_autograd(v.with_tensors(sdf_p, feat_p), inv_s, _dev_rays(ex), cfg, want_grad_samples=True,
                               t_rand=None if t_rand is None else t_rand.to(D0), bkgd_rays=bk.to(D0))
    sum((out[k] * G[k].to(D0)).sum() for k in G).backward()
    return vol, ex, cfg, t_rand, bk, G, out, sdf_p, feat_p, inv_s


@pytest.mark.parametrize("scatter", ["atomic", "binned"])
@pytest.mark.parametrize("deg,act,jitter,sample_pos,S", [
    (1, 'relu', abi.JITTER_NONE, 0, 32), (2, 'relu', abi.JITTER_SINGLE, 1, 32), (2, 'sigmoid', abi.JITTER_PER_BIN, 0, 32),
    (1, 'sigmoid', abi.JITTER_NONE, 0, 100), (2, 'relu', abi.JITTER_NONE, 0, 256), (2, 'sigmoid', abi.JITTER_SINGLE, 0, 300),
    (0, 'sigmoid', abi.JITTER_SINGLE, 0, 32)])
def test_sh_render_backward_vs_float64_autograd(hip, deg, act, jitter, sample_pos, S, scatter):
    """random upstream gradients on rgb, depth, acc, weights (and per-sample sdf / grad), no sample left out; the bounds of
    test_render_backward_vs_float64_autograd"""
    vol, ex, cfg, t_rand, bk, G, out, sdf_p, feat_p, inv_s = _backward_case(deg, act, jitter, sample_pos, S, scatter)
    dd = torch.float64
    sdf64, feat64 = vol.sdf.to(dd).requires_grad_(True), vol.feat.to(dd).requires_grad_(True)
    inv_s64 = torch.tensor(cfg.inv_s, dtype=dd, requires_grad=True)
    ref = compose64(vol.mapping, sdf64, feat64, deg, act, ex, cfg, inv_s64, t_rand, bk)
    for k in G:
        assert torch.allclose(out[k].detach().cpu().double(), ref[k].detach(), rtol=2e-3, atol=2e-4), k
    sum((ref[k] * G[k].to(dd)).sum() for k in G).backward()
    n_coef = sh.n_coef(deg)
    e_sdf = _rel_l2(sdf_p.grad.cpu().double(), sdf64.grad)
    e_f = _rel_l2(feat_p.grad.cpu().double()[..., :n_coef], feat64.grad[..., :n_coef])
    e_s = abs(inv_s.grad.item() - inv_s64.grad.item()) / (abs(inv_s64.grad.item()) + 1e-12)
    print(f"\n[sh bwd deg {deg} {act} S {S} {scatter}] sdf {e_sdf:.3e} feat {e_f:.3e} inv_s {e_s:.3e}")
    assert e_sdf < 2e-3, f"d/d sdf_vol rel L2 {e_sdf:.3e}"
    assert (sdf_p.grad.cpu().double() - sdf64.grad).abs().max() < 2e-2 * sdf64.grad.abs().max()
    assert feat64.grad[..., :n_coef].abs().max() > 0
    assert e_f < 2e-3, f"d/d feat_vol rel L2 {e_f:.3e}"
    if feat_p.shape[-1] > n_coef:
        assert feat_p.grad[..., n_coef:].abs().max() == 0          # the pad channel (27 at degree 2) is exactly zero
        assert feat64.grad[..., n_coef:].abs().max() == 0
    assert e_s < 5e-2, f"d/d inv_s rel {e_s:.3e} ({inv_s.grad.item()} vs {inv_s64.grad.item()})"


# (the degree-2 cases keep the ids they had while they were the only ones)
@pytest.mark.parametrize("deg,act,scatter", [(2, 'relu', "atomic"), (2, 'relu', "binned"), (1, 'relu', "atomic"), (1, 'relu', "binned"),
                                             (0, 'sigmoid', "atomic"), (0, 'sigmoid', "binned")],
                         ids=["atomic", "binned", "1-relu-atomic", "1-relu-binned", "0-sigmoid-atomic", "0-sigmoid-binned"])
def test_sh_render_backward_under_the_upscale_mapping(hip, deg, act, scatter):
    vol, ex, cfg, t_rand, bk, G, out, sdf_p, feat_p, inv_s = _backward_case(deg, act, abi.JITTER_NONE, 0, 100, scatter, upscale=True)
    dd = torch.float64
    sdf64, feat64 = vol.sdf.to(dd).requires_grad_(True), vol.feat.to(dd).requires_grad_(True)
    inv_s64 = torch.tensor(cfg.inv_s, dtype=dd, requires_grad=True)
    ref = compose64(vol.mapping, sdf64, feat64, deg, act, ex, cfg, inv_s64, t_rand, bk)
    sum((ref[k] * G[k].to(dd)).sum() for k in G).backward()
    assert _rel_l2(sdf_p.grad.cpu().double(), sdf64.grad) < 2e-3
    assert _rel_l2(feat_p.grad.cpu().double(), feat64.grad) < 2e-3
    assert feat64.grad.abs().max() > 0
    if feat_p.shape[-1] > sh.n_coef(deg):
        assert feat_p.grad[..., sh.n_coef(deg):].abs().max() == 0          # the pad channel (27 at degree 2, 3 at degree 0)


@pytest.mark.parametrize("scatter", ["atomic", "binned"])
def test_sh_render_backward_zero_upstream(hip, scatter):
    _, _, _, _, _, _, _, sdf_p, feat_p, inv_s = _backward_case(2, 'sigmoid', abi.JITTER_NONE, 0, 100, scatter, zero=True)
    assert sdf_p.grad.abs().max() == 0 and feat_p.grad.abs().max() == 0 and inv_s.grad.abs().max() == 0


LOG = os.path.join(ROOT, "parity_out", "render_sh_parity.jsonl")


@pytest.mark.parametrize("act", ['relu', 'sigmoid'])
def test_sh_render_backward_binned_vs_atomic_at_training_shape(hip, act):
    """the rays, samples and 257 x 257 x 25 volume of test_render_backward_binned_vs_atomic_at_training_shape at degree 2:
    the 64-byte-record binned scatter (basis expanded in the brick kernel) and the per-sample row atomics give the same
    gradients; the bounds of that test.  Measured errors go to parity_out/render_sh_parity.jsonl (profiles/sh_render_bwd_parity.jsonl)."""
    rays = sy.make_rays("cfg5")
    rg = RaySet(img2lidar=rays.img2lidar.to(D0), nx=rays.nx, ny=rays.ny, sx=rays.sx, sy=rays.sy)
    vol = sy.make_volume("cfg5", n_rgb=3, sh_deg=2, sh_act=act).to(D0)
    res = {}
    for mode in ("atomic", "binned"):
        cfg = sy.make_render_config("cfg5")
        cfg.bwd_scatter = mode
        inv_s = torch.tensor([float(cfg.inv_s)], device=D0, requires_grad=True)
        sdf, feat = vol.sdf.detach().clone().requires_grad_(True), vol.feat.detach().clone().requires_grad_(True)
        out = render_rays_autograd(vol.with_tensors(sdf, feat), inv_s, rg, cfg)
        loss = out['depth'].mean() + out['sdf'].abs().mean() * 0.1 + (out['grad'].norm(dim=-1) - 1).square().mean() * 0.1 + \
            (out['weights'] * torch.linspace(0, 1, out['weights'].shape[-1], device=D0)).sum(-1).mean() + \
            (out['rgb'] * torch.tensor([1.0, -0.5, 0.25], device=D0)).mean()
        loss.backward()
        res[mode] = (sdf.grad, feat.grad, inv_s.grad)
    a, b = res["atomic"], res["binned"]
    m = dict(act=act, sh_deg=2, n_rays=rg.n_rays, n_samples=256,
             sdf_l2=_rel_l2(b[0].double(), a[0].double()), sdf_max=((b[0] - a[0]).abs().max() / a[0].abs().max()).item(),
             feat_l2=_rel_l2(b[1].double(), a[1].double()), feat_max=((b[1] - a[1]).abs().max() / a[1].abs().max()).item(),
             inv_s_rel=abs(b[2].item() - a[2].item()) / abs(a[2].item()))
    print("\n[sh binned vs atomic]", m)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(m) + "\n")
    except OSError:
        pass
    assert a[0].abs().max() > 0 and a[1][..., :27].abs().max() > 0
    assert m['sdf_l2'] < 1e-5 and m['sdf_max'] <= 1e-4, m
    assert m['feat_l2'] < 1e-5 and m['feat_max'] <= 1e-4, m
    assert a[1][..., 27].abs().max() == 0 and b[1][..., 27].abs().max() == 0
    assert abs(b[2].item() - a[2].item()) <= 1e-3 * abs(a[2].item()) + 1e-6
