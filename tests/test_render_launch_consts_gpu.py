"""GPU: the skip marcher's launch constants and its 3-D launch grid (csrc/render_fwd.hip, so_launch_consts).

The code-ahead skip marcher (so_march_fast_ahead, the default route of an SDF-only launch with a brick) takes what is
constant for a launch — per axis k1 = size0 / range0 and k0 = (off0 + off1) - start * k1, the skip unit, the near-face
margin, (float)S, two byte offsets — from a struct the host fills, and its pixel-grid kernels read tile and camera from
blockIdx on a grid (tiles_x, tiles_y, n_cams).  ``RenderConfig(ahead=False)`` runs so_march_fast, which computes all of it on
the device from the launch arguments and maps the linear block index with two divisions: an independent route through
the same library, and the reference here.  All five outputs are compared with torch.equal.

The shapes are ones at which a wrong constant or a wrong tile map shows:
  * the 12 x 10 x 6 volume of tests/test_render_face_cold_gpu.py (half axes: off0 = 0; no cell size is a binary fraction)
    under an AABB a little inside it, whose corners and extents are not float32 numbers, and a 9 x 7 x 5 volume with
    centred axes (off0 != 0, so k0 has both terms) under its own box;
  * S in {1, 7, 33, 128}; inv_s in {20, 200}, by value and through ``inv_s_dev`` (with another value in the host field:
    a launch that read the host's would differ from the reference, which gets the value itself);
  * lattices 37 x 19 (3 x 2 tiles) and 16 x 33 (1 x 3 tiles): tiles_x != tiles_y, edge tiles on both axes, with 1 and 3
    cameras whose matrices differ; explicit rays for one case of each volume;
  * one lattice of 1 x 1 pixels with 65 537 cameras on a 6 x 5 x 4 volume: more than gridDim.z holds, so the launch takes
    the step-by-step march.
Every launch is given the brick workspace, whatever its size (render_rays allocates one only for large batches), so that
every case takes the route under test.  No case is vacuous: some rays end with acc > 0.5 and some with acc < 0.5.
"""
import functools
import math

import numpy as np
import pytest
import torch

from selfocc_amd import synthetic as sy
from selfocc_amd._lib import check, current_stream, lib, ptr
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import RaySet, RenderConfig, SDFVolume, _brick_workspace, marshal_render_args

pytestmark = pytest.mark.gpu

KEYS = ("depth", "acc", "max_depth", "nears", "fars")
S_LIST, INV_S_LIST, HOWS = (1, 7, 33, 128), (20.0, 200.0), ("value", "device")
LATTICES = ((37, 19), (16, 33))
FOCAL = 20.0

# name -> (mapping, render AABB, ground level, boxes, three camera poses (position, yaw in degrees) outside the AABB)
SCENES = {
    "v12": (dict(nonlinear_mode='linear', h_size=[11, 0], h_range=[5.2, 0], h_half=True, w_size=[9, 0], w_range=[4.4, 0],
                 w_half=True, d_size=[5, 0], d_range=[-1.0, 1.2, 1.2]),
            (0.1, 0.3, -0.9, 4.3, 5.1, 1.1), -0.2,
            (((2.6, 3.2, 0.1), (0.4, 0.5, 0.5)), ((1.1, 4.0, 0.3), (0.5, 0.4, 0.7)), ((3.6, 1.2, 0.0), (0.4, 0.4, 0.4))),
            (((-1.5, 2.6, 0.2), 0.0), ((2.2, -1.5, 0.3), 90.0), ((5.5, 6.0, 0.1), 225.0))),
    "v9": (dict(nonlinear_mode='linear', h_size=[4, 0], h_range=[2.3, 0], h_half=False, w_size=[3, 0], w_range=[1.7, 0],
                w_half=False, d_size=[4, 0], d_range=[-0.7, 1.1, 1.1]),
           (-1.7, -2.3, -0.7, 1.7, 2.3, 1.1), -0.2,
           (((0.5, 0.9, 0.1), (0.4, 0.5, 0.5)), ((-0.8, -1.0, 0.2), (0.5, 0.4, 0.6))),
           (((-3.0, 0.1, 0.2), 0.0), ((0.2, -3.5, 0.3), 90.0), ((3.0, 3.5, 0.1), 225.0))),
    "v6": (dict(nonlinear_mode='linear', h_size=[5, 0], h_range=[2.6, 0], h_half=True, w_size=[4, 0], w_range=[2.2, 0],
                w_half=True, d_size=[3, 0], d_range=[-0.7, 0.8, 0.8]),
           (0.0, 0.0, -0.7, 2.2, 2.6, 0.8), -0.2, (((1.2, 1.5, 0.1), (0.4, 0.5, 0.5)),), ()),
}
SHAPES = {"v12": (12, 10, 6), "v9": (9, 7, 5), "v6": (6, 5, 4)}


@functools.lru_cache(maxsize=None)
def volume(name):
    """synthetic.make_volume's recipe: a ground plane, boxes, noise"""
    m = GridMeterMapping(**SCENES[name][0])
    xyz = sy.grid_points_meter(m)
    sdf = xyz[..., 2] - SCENES[name][2]
    for c, half in SCENES[name][3]:
        q = (xyz - torch.tensor(c)).abs() - torch.tensor(half)
        sdf = torch.minimum(sdf, torch.linalg.norm(q.clamp_min(0.0), dim=-1) + q.max(dim=-1).values.clamp_max(0.0))
    sdf = sdf + 0.05 * torch.randn(sdf.shape, generator=torch.Generator().manual_seed(5))
    assert tuple(sdf.shape) == SHAPES[name]
    return SDFVolume(m, sdf.contiguous().float()).to(torch.device("cuda:0"))


def camera(pos, yaw_deg, nx, ny):
    """img2lidar of a level pinhole at `pos` looking along yaw (synthetic.make_cameras' convention)"""
    yaw = math.radians(yaw_deg)
    fwd = np.array([math.cos(yaw), math.sin(yaw), 0.0])
    right = np.array([math.sin(yaw), -math.cos(yaw), 0.0])
    down = np.array([0.0, 0.0, -1.0])
    K = np.array([[FOCAL, 0, nx / 2.0, 0], [0, FOCAL, ny / 2.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([right, down, fwd], axis=1)
    c2w[:3, 3] = pos
    return c2w @ np.linalg.inv(K)


def lattice(name, nx, ny, n_cams):
    mats = np.stack([camera(pos, yaw, nx, ny) for pos, yaw in SCENES[name][4][:n_cams]])
    return RaySet(img2lidar=torch.tensor(mats, dtype=torch.float32), nx=nx, ny=ny, sx=1.0, sy=1.0)


def many_cameras(n):
    """n pinholes of one pixel each around the v6 volume: every camera looks at a point near the box's centre from 3 m away,
    pitched between 40 degrees down and 40 degrees up (a ray that runs down meets the ground, one that runs up meets nothing)"""
    i = np.arange(n, dtype=np.float64)
    yaw, pitch = 2.0 * math.pi * ((i * 0.61803398875) % 1.0), np.radians(-40.0 + 80.0 * ((i * 0.3819660113) % 1.0))
    fwd = np.stack([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)], 1)
    right = np.stack([np.sin(yaw), -np.cos(yaw), np.zeros(n)], 1)
    down = np.cross(fwd, right)
    target = np.array([1.1, 1.3, 0.05]) + 0.3 * np.stack([np.cos(7.0 * yaw), np.sin(5.0 * yaw), 0.5 * np.sin(3.0 * yaw)], 1)
    c2w = np.tile(np.eye(4), (n, 1, 1))
    c2w[:, :3, 0], c2w[:, :3, 1], c2w[:, :3, 2], c2w[:, :3, 3] = right, down, fwd, target - 3.0 * fwd
    K = np.array([[FOCAL, 0, 0.5, 0], [0, FOCAL, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    return RaySet(img2lidar=torch.tensor(c2w @ np.linalg.inv(K), dtype=torch.float32), nx=1, ny=1, sx=1.0, sy=1.0)


def launch(vol, rays, cfg):
    """render_rays with the brick workspace whatever the size of the batch"""
    a, out, _keep = marshal_render_args(vol, rays, cfg)
    a.sdf_brick = ptr(_brick_workspace(vol.sdf))
    check(lib().selfocc_render_fwd(a, current_stream(vol.sdf.device)), "selfocc_render_fwd")
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in KEYS}


def on_gpu(rays):
    d = torch.device("cuda:0")
    if rays.pixel_grid:
        return RaySet(img2lidar=rays.img2lidar.to(d), nx=rays.nx, ny=rays.ny, sx=rays.sx, sy=rays.sy)
    return RaySet(origins=rays.origins.to(d), dirs=rays.dirs.to(d), dir_norm=rays.dir_norm.to(d))


@functools.lru_cache(maxsize=None)
def rays_of(name, mode, nx, ny, n_cams):
    r = lattice(name, nx, ny, n_cams)
    return on_gpu(sy.explicit_rays(r) if mode == "explicit" else r)


@functools.lru_cache(maxsize=None)
def reference(name, mode, nx, ny, n_cams, S, inv_s):
    """the step-by-step march, inv_s by value"""
    return launch(volume(name), rays_of(name, mode, nx, ny, n_cams),
                  RenderConfig(aabb=SCENES[name][1], n_samples=S, inv_s=inv_s, ahead=False))


def run(name, mode, nx, ny, n_cams, S, inv_s, how):
    if how == "device":     # the kernels must read the device's value: the host field holds another one
        cfg = RenderConfig(aabb=SCENES[name][1], n_samples=S, inv_s=0.5 * inv_s,
                           inv_s_dev=torch.tensor([inv_s], dtype=torch.float32, device="cuda:0"))
    else:
        cfg = RenderConfig(aabb=SCENES[name][1], n_samples=S, inv_s=inv_s)
    return launch(volume(name), rays_of(name, mode, nx, ny, n_cams), cfg)


def compare(got, ref, case):
    acc = ref["acc"]
    hi, lo = int((acc > 0.5).sum()), int((acc < 0.5).sum())
    bad = {k: int((got[k].view(torch.int32) != ref[k].view(torch.int32)).sum()) for k in KEYS}
    print(f"[launch-consts] {case}: rays {acc.numel()}, acc > 0.5: {hi}, acc < 0.5: {lo}; differing values {bad}")
    assert hi > 0 and lo > 0, (case, hi, lo)
    for k in KEYS:
        assert torch.equal(got[k], ref[k]), (case, k, bad[k])
    assert torch.isfinite(got["depth"]).all() and torch.isfinite(got["acc"]).all()


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("inv_s", INV_S_LIST)
@pytest.mark.parametrize("S", S_LIST)
@pytest.mark.parametrize("n_cams", (1, 3))
@pytest.mark.parametrize("nx,ny", LATTICES)
@pytest.mark.parametrize("name", ("v12", "v9"))
def test_pixel_grid_equals_step_by_step(hip, name, nx, ny, n_cams, S, inv_s, how):
    case = (name, nx, ny, n_cams, S, inv_s, how)
    compare(run(name, "pixgrid", nx, ny, n_cams, S, inv_s, how), reference(name, "pixgrid", nx, ny, n_cams, S, inv_s), case)


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", ("v12", "v9"))
def test_explicit_rays_equal_step_by_step(hip, name, how):
    case = (name, "explicit", 37, 19, 3, 33, 20.0, how)
    compare(run(name, "explicit", 37, 19, 3, 33, 20.0, how), reference(name, "explicit", 37, 19, 3, 33, 20.0), case)


def test_more_cameras_than_the_grid_holds(hip):
    """65 537 cameras: gridDim.z ends at 65 535, so the default route launches the step-by-step march"""
    rays = on_gpu(many_cameras(65537))
    kw = dict(aabb=SCENES["v6"][1], n_samples=16, inv_s=20.0)
    got = launch(volume("v6"), rays, RenderConfig(**kw))
    ref = launch(volume("v6"), rays, RenderConfig(ahead=False, **kw))
    assert got["acc"].numel() == 65537
    compare(got, ref, ("v6", 1, 1, 65537, 16, 20.0, "value"))
