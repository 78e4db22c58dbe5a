"""GPU: the rendered normal in one launch (selfocc_render_normal).

The oracle of every case is `normal_vis_reference` applied to the `weights` / `grad` that `render_rays(per_sample=True,
want_grad_samples=True)` — the sample-parallel kernel every earlier version ships, not the kernel under test — returns for the
same inputs.  The three channels must be EQUAL, bit for bit, on every ray: no tolerance, no ray left out.  Every case first
asserts, on the oracle's numbers alone, that the frame is not all sky and that a ray misses the box.

Scenes.  Linear mapping: the `synthetic` cfg1 volume (32 x 32 x 4 grid points); camera 0 stands inside the box just above the
ground and looks down, camera 1 stands 8 m in front of its x = 0 face, so that its top and bottom pixel rows pass above / below
the box by more than a cell.  Upscale mapping: the scene of tests/test_mapping_upscale_gpu.py (ground, cylindrical wall, ceiling
on NeuSHead's default 321 x 321 x 31 lattice), camera 0 inside, camera 1 50 m in front of the x = -80 face.  Pixel-grid rays are
a 10 x 6 lattice of the two cameras (not a multiple of the 16 x 16 tile); the explicit rays are a 16 x 8 lattice of the same cameras expanded on the host plus one
ray straight down: 257, not a multiple of the 256 rays of a block."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import oracle
from selfocc_amd import abi, synthetic as sy
from selfocc_amd._lib import lib, ptr, current_stream
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import (RaySet, RenderConfig, SDFVolume, marshal_render_args, normal_vis_reference, render_normal_vis,
                                render_rays, upsample_edges)

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
SAMPLE_COUNTS = [1, 2, 63, 64, 65, 128, 129, 256]       # the segment / pass boundaries of the scan replay (seg_per_pass 1, 2, 4)
POSITIONS = {'start': abi.SAMPLE_AT_START, 'mid': abi.SAMPLE_AT_MID}
JITTERS = {'none': abi.JITTER_NONE, 'single': abi.JITTER_SINGLE, 'per_edge': abi.JITTER_PER_BIN}
INV_S = 20.0


def _pinhole(position, pitch_deg):
    """img2lidar of the cfg1 pinhole (focal 60 on a 64 x 64 image) at `position`, looking along +x, pitched down by pitch_deg"""
    K = np.array([[60.0, 0, 32, 0], [0, 60.0, 32, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    c, s = np.cos(np.deg2rad(pitch_deg)), np.sin(np.deg2rad(pitch_deg))
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([[0.0, -1.0, 0.0], [-s, 0.0, -c], [c, 0.0, -s]], axis=1)      # right, down, forward
    c2w[:3, 3] = position
    return c2w @ np.linalg.inv(K)


def _cameras(kind):
    """(2, 4, 4) img2lidar.  Camera 0 stands inside the volume and looks 35 degrees down (half field of view 28 degrees); in the
    linear scene it hangs 0.25 m above the ground (z = -0.55), so that even the one sample of S = 1, taken at the camera, lies
    within half a step of the surface and carries weight.  Camera 1 stands in front of the volume and looks level, so that
    its outer rows pass above and below the box."""
    pos = [(6.4, 6.4, -0.3), (-8.0, 6.4, 0.5)] if kind == 'linear' else [(0.3, -0.2, 0.5), (-130.0, 0.0, 0.5)]
    return torch.tensor(np.stack([_pinhole(pos[0], 35.0), _pinhole(pos[1], 0.0)]), dtype=torch.float32)


_SCENES = {}


def _scene(kind):
    """(volume on the device, aabb) — built once per mapping kind and never changed"""
    if kind not in _SCENES:
        if kind == 'linear':
            vol, aabb = sy.make_volume("cfg1"), sy.CONFIGS["cfg1"]["aabb"]
        else:
            import test_mapping_upscale_gpu as mu
            vol, aabb = mu._volume(GridMeterMapping(**mu.HEAD_UPSCALE), 0, 0), mu.AABB
        _SCENES[kind] = (vol.to(D0), tuple(aabb))
    return _SCENES[kind]


def _rays(kind, pixel):
    cams = _cameras(kind)
    if pixel:
        return RaySet(img2lidar=cams.to(D0), nx=10, ny=6, sx=6.4, sy=64 / 6)
    e = sy.explicit_rays(RaySet(img2lidar=cams, nx=16, ny=8, sx=4.0, sy=8.0))
    ctr = cams[0, :3, 3]
    rs = RaySet(origins=torch.cat([e.origins, ctr[None]]).contiguous().to(D0),
                dirs=torch.cat([e.dirs, torch.tensor([[0.0, 0.0, -1.0]])]).contiguous().to(D0),
                dir_norm=torch.cat([e.dir_norm, torch.tensor([1.5])]).contiguous().to(D0))
    assert rs.n_rays == 257
    return rs


def _misses_the_box(rays, aabb):
    """float64 slab test of every ray against the collider box: True where the ray never enters it"""
    e = sy.explicit_rays(rays.cpu()) if rays.pixel_grid else rays.cpu()
    o, d = e.origins.double().numpy(), e.dirs.double().numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        t0, t1 = (np.asarray(aabb[:3]) - o) / d, (np.asarray(aabb[3:]) - o) / d
    tn, tf = np.nanmax(np.minimum(t0, t1), -1), np.nanmin(np.maximum(t0, t1), -1)
    return torch.from_numpy(tf < np.maximum(tn, 0.0))


def _t_rand(jitter, n_rays, S, seed=11):
    g = torch.Generator().manual_seed(seed)
    if jitter == abi.JITTER_SINGLE:
        return torch.rand(n_rays, generator=g).to(D0)
    if jitter == abi.JITTER_PER_BIN:
        return torch.rand(n_rays, S + 1, generator=g).to(D0)
    return None


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check(vol, rays, cfg, aabb, label, t_rand=None, edges=None, min_acc=True):
    """the kernel against the definition on the per-sample outputs of the same arguments; returns (got, want, per-sample dict)"""
    per = render_rays(vol, rays, cfg, per_sample=True, want_grad_samples=True, t_rand=t_rand, edges=edges)
    w, g = per['weights'].cpu(), per['grad'].cpu()
    want = normal_vis_reference(w, g)
    # what the oracle must show for the comparison to mean something
    acc = w.sum(1)
    if min_acc:
        assert (acc > 0.05).float().mean() > 0.25, f"{label}: only {(acc > 0.05).float().mean():.2f} of the rays accumulate: all sky"
    miss = _misses_the_box(rays, aabb)
    assert miss.any(), f"{label}: no ray misses the box"
    got = render_normal_vis(vol, rays, cfg, t_rand=t_rand, edges=edges)
    assert got.shape == (rays.n_rays, 3) and got.dtype == torch.float32 and got.device.type == 'cuda'
    gc = got.cpu()
    bad = (_bits(gc) != _bits(want)).any(1).nonzero().flatten().tolist()
    assert not bad, f"{label}: normal_vis differs on {len(bad)} of {rays.n_rays} rays, first {bad[:4]}: got {gc[bad[:4]].tolist()} " \
                    f"want {want[bad[:4]].tolist()}, max |diff| {(gc - want).abs().max():.3e}"
    assert torch.equal(gc, want)
    half = (gc[miss] == 0.5).all(1)
    assert half.any(), f"{label}: none of the {int(miss.sum())} rays that miss the box returns exactly (0.5, 0.5, 0.5)"
    return gc, want, per


@pytest.mark.parametrize("pixel", [True, False], ids=["pixgrid", "explicit"])
@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_normal_equals_the_reference_on_per_sample_outputs(hip, S, pixel):
    vol, aabb = _scene('linear')
    rays = _rays('linear', pixel)
    assert rays.n_rays == (120 if pixel else 257)
    moved = 0
    for pname, pos in POSITIONS.items():
        for jname, jit in JITTERS.items():
            cfg = RenderConfig(aabb=aabb, n_samples=S, inv_s=INV_S, sample_pos=pos, jitter_mode=jit)
            got, _, _ = _check(vol, rays, cfg, aabb, f"S={S} {pname} {jname} {'pixgrid' if pixel else 'explicit'}",
                               t_rand=_t_rand(jit, rays.n_rays, S))
            moved += int(((got - 0.5).abs() > 0.05).any(1).sum())
    assert moved > 0, "no ray shows a normal: the scene says nothing"


@pytest.mark.parametrize("pixel", [True, False], ids=["pixgrid", "explicit"])
@pytest.mark.parametrize("S", [65, 256])
def test_normal_on_the_upscale_mapping(hip, S, pixel):
    vol, aabb = _scene('upscale')
    assert vol.mapping.to_abi().kind == abi.MAP_UPSCALE
    rays = _rays('upscale', pixel)
    for pname, pos in POSITIONS.items():
        for jname, jit in JITTERS.items():
            cfg = RenderConfig(aabb=aabb, n_samples=S, inv_s=INV_S, sample_pos=pos, jitter_mode=jit)
            _check(vol, rays, cfg, aabb, f"upscale S={S} {pname} {jname} {'pixgrid' if pixel else 'explicit'}",
                   t_rand=_t_rand(jit, rays.n_rays, S))


@pytest.mark.parametrize("pixel", [True, False], ids=["pixgrid", "explicit"])
def test_normal_on_explicit_edges_from_upsampling(hip, pixel):
    """S_tot = 64 + 4 * 4 = 80 edges per ray from upsample_edges travel in the t_rand slot (SO_JITTER_EDGES)"""
    vol, aabb = _scene('linear')
    rays = _rays('linear', pixel)
    cfg = RenderConfig(aabb=aabb, n_samples=64, inv_s=INV_S)
    edges = upsample_edges(vol, rays, cfg, 16, 4, 16.0)
    assert edges.shape == (rays.n_rays, 81)
    uniform = torch.linspace(0, 1, 81, device=D0)
    assert not torch.allclose(edges, uniform.expand_as(edges)), "the field must move some samples"
    _check(vol, rays, cfg, aabb, f"edges S_tot=80 {'pixgrid' if pixel else 'explicit'}", edges=edges)


def test_flat_sdf_gives_exactly_one_half(hip):
    """a constant volume has zero trilinear gradients (every corner difference is an exact 0), so every n_i is 0 under the
    1e-12 clamp and the result is exactly 0.5 although the weights are not zero"""
    vol, aabb = _scene('linear')
    flat = SDFVolume(vol.mapping, torch.zeros_like(vol.sdf))
    for pixel in (True, False):
        rays = _rays('linear', pixel)
        cfg = RenderConfig(aabb=aabb, n_samples=65, inv_s=INV_S, sample_pos=abi.SAMPLE_AT_MID)
        got, _, per = _check(flat, rays, cfg, aabb, "flat", min_acc=False)
        assert (per['weights'] > 0).any() and torch.count_nonzero(per['grad']) == 0
        assert (got == 0.5).all()


def test_inv_s_comes_from_the_device_copy(hip):
    vol, aabb = _scene('linear')
    rays = _rays('linear', True)
    cfg = RenderConfig(aabb=aabb, n_samples=64, inv_s=INV_S)
    want = render_normal_vis(vol, rays, dataclasses.replace(cfg, inv_s=200.0))
    cfg_dev = dataclasses.replace(cfg, inv_s=1.0, inv_s_dev=torch.tensor([200.0], device=D0))       # the host value must lose
    got, _, _ = _check(vol, rays, cfg_dev, aabb, "inv_s_dev")
    assert torch.equal(got, want.cpu())
    assert not torch.equal(render_normal_vis(vol, rays, dataclasses.replace(cfg, inv_s=1.0)).cpu(), got)


def test_normal_against_the_c_oracle(hip):
    """the independent C march (oracle/), composed on the host as tests/test_head_gpu.py does, within that test's 1e-4"""
    vol, aabb = _scene('linear')
    rays = _rays('linear', True)
    cfg = RenderConfig(aabb=aabb, n_samples=65, inv_s=INV_S)
    refs = oracle.render_fwd(SDFVolume(vol.mapping, vol.sdf.cpu()), rays.cpu(), cfg, per_sample=True, want_grad_samples=True)
    g = refs['grad']
    want = ((refs['weights'].unsqueeze(-1) * (g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12))).sum(1) + 1.0) / 2.0
    got = render_normal_vis(vol, rays, cfg).cpu()
    assert ((want - 0.5).abs() > 0.05).any()
    assert got.shape == want.shape and (got - want).abs().max() < 1e-4


def test_a_refused_call_leaves_the_output_alone(hip):
    vol, aabb = _scene('linear')
    rays = _rays('linear', False)
    cfg = RenderConfig(aabb=aabb, n_samples=64, inv_s=INV_S)
    N = rays.n_rays
    sentinel = -7.25
    buf = torch.full((N * 3 + 64,), sentinel, device=D0)
    a, _o, _keep = marshal_render_args(SDFVolume(vol.mapping, vol.sdf), rays, cfg, inputs_only=True)
    na = abi.SoRenderNormalArgs()
    na.fwd = a
    na.normal_vis = ptr(buf)
    st = current_stream(D0)
    for field, value, word in (('n_samples', 0, b"n_samples"), ('sample_pos', 2, b"sample_pos"), ('sdf_vol', None, b"sdf_vol")):
        bad = abi.SoRenderNormalArgs()
        bad.fwd, bad.normal_vis = a, ptr(buf)
        setattr(bad.fwd, field, value)
        assert lib().selfocc_render_normal(bad, st) < 0 and word in lib().selfocc_last_error()
    none = abi.SoRenderNormalArgs()
    none.fwd = a
    assert lib().selfocc_render_normal(none, st) < 0 and b"normal_vis" in lib().selfocc_last_error()
    torch.cuda.synchronize()
    assert (buf == sentinel).all(), "a refused call wrote to the output"
    assert lib().selfocc_render_normal(na, st) == 0, lib().selfocc_last_error()
    torch.cuda.synchronize()
    assert (buf[:N * 3] != sentinel).all() and (buf[N * 3:] == sentinel).all()        # every ray written, nothing past the end
    assert torch.equal(buf[:N * 3].reshape(N, 3), render_normal_vis(vol, rays, cfg))


def test_no_rays_is_no_launch(hip):
    vol, aabb = _scene('linear')
    none = RaySet(origins=torch.zeros(0, 3, device=D0), dirs=torch.zeros(0, 3, device=D0), dir_norm=torch.zeros(0, device=D0))
    assert render_normal_vis(vol, none, RenderConfig(aabb=aabb, n_samples=64, inv_s=INV_S)).shape == (0, 3)


def test_the_call_ignores_features_background_and_march_switches(hip):
    vol, aabb = _scene('linear')
    rays = _rays('linear', True)
    cfg = RenderConfig(aabb=aabb, n_samples=64, inv_s=INV_S)
    want = render_normal_vis(vol, rays, cfg)
    full = sy.make_volume("cfg1", n_rgb=3, n_sem=5).to(D0)
    assert full.feat is not None and torch.equal(full.sdf, vol.sdf)
    odd = dataclasses.replace(cfg, bkgd_mode=abi.BKGD_PER_RAY, clamp_rgb=True, exact=True, brick=False, skip=False, face_safe=False,
                              ahead=False, depth_div_norm=False)
    assert torch.equal(render_normal_vis(full, rays, odd), want)


# ---- the head -----------------------------------------------------------------------------------------------------
def _head_and_inputs(**kw):
    from test_head_gpu import make_head, make_inputs
    rep, metas, _ = make_inputs()
    head = make_head(render_bkgd='white', **kw).eval()
    with torch.no_grad():
        head.prepare(rep, metas)
    return head, metas


SIGNAL = 1e-4       # the head's frame must show normals at least 100 x the bound of the comparison away from 0.5 (the random
                    # field of tests/test_head_gpu.py is soft: its normals reach ~1e-3)


def _per_sample_route(head, metas):
    """NeuSHead._normal_vis, the chunked per-sample route this change does not touch, on the head's own rays"""
    vol = head.model.field.volume.detached()
    rays, _pix, num_cams, num_rays = head._rays(metas, vol.sdf.device)
    cfg = head._render_cfg(False)
    cfg.inv_s_dev = head.model.field.inv_s_device()
    return head._normal_vis(vol, rays, cfg, chunk_rays=25).reshape(1, num_cams, num_rays, 3)


def test_head_render_fills_vis_normal_from_the_launch(hip):
    os.environ['eval'] = 'true'
    try:
        head, metas = _head_and_inputs()
        with torch.no_grad():
            off = head.render(metas)
            on = head.render(metas, vis_normal=True)
            want = _per_sample_route(head, metas)
        assert head.render_normal is False and torch.count_nonzero(off['vis_normal'][0]) == 0       # the default: zeros, no launch
        got = on['vis_normal'][0]
        assert got.shape == want.shape == (1, 2, 60, 3)
        print(f"signal {float((want - 0.5).abs().max()):.3e}  difference {float((got - want).abs().max()):.3e}")
        assert (want - 0.5).abs().max() > SIGNAL
        assert (got - want).abs().max() < 1e-6
        for k in off:                                         # the other outputs do not notice the extra launch
            if k != 'vis_normal':
                a, b = on[k], off[k]
                assert torch.equal(a[0], b[0]) if isinstance(a, list) else torch.equal(a, b), k
        # the constructor flag is the same switch
        from test_head_gpu import make_head, make_inputs
        rep, metas2, _ = make_inputs()
        flagged = make_head(render_bkgd='white', render_normal=True).eval()
        with torch.no_grad():
            flagged.prepare(rep, metas2)
            assert torch.equal(flagged.render(metas2)['vis_normal'][0], got)
            assert torch.count_nonzero(flagged.render(metas2, vis_normal=False)['vis_normal'][0]) == 0
    finally:
        os.environ['eval'] = 'false'


def test_upsampled_head_fills_vis_normal_chunk_by_chunk(hip):
    os.environ['eval'] = 'true'
    try:
        head, metas = _head_and_inputs(num_samples=16, num_samples_importance=16, num_up_sample_steps=4)
        assert head.up_steps == 4 and head.total_samples == 32
        n_rays = 2 * 60
        head.up_edge_bytes = n_rays * 33 * 4 // 3               # three chunks of rows
        assert -(-(n_rays * 33 * 4) // head.up_edge_bytes) >= 2
        with torch.no_grad():
            got = head.render(metas, vis_normal=True)['vis_normal'][0]
            want = _per_sample_route(head, metas)
            assert torch.count_nonzero(head.render(metas)['vis_normal'][0]) == 0
        assert got.shape == want.shape == (1, 2, 60, 3)
        print(f"signal {float((want - 0.5).abs().max()):.3e}  difference {float((got - want).abs().max()):.3e}")
        assert (want - 0.5).abs().max() > SIGNAL
        assert (got - want).abs().max() < 1e-6
    finally:
        os.environ['eval'] = 'false'


def test_head_render_with_vis_normal_never_syncs(hip):
    os.environ['eval'] = 'true'
    try:
        head, metas = _head_and_inputs()
        with torch.no_grad():
            head.render(metas, vis_normal=True)               # first call: lazy initialisation may synchronise
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                out = head.render(metas, vis_normal=True)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert torch.isfinite(out['vis_normal'][0]).all() and torch.count_nonzero(out['vis_normal'][0] - 0.5) > 0
    finally:
        os.environ['eval'] = 'false'
