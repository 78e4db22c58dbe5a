"""GPU: the dispatch order of the pixel-grid skip marcher (csrc/render_fwd.hip, render_fwd_pixgrid of so_launch_consts).

The kernel is launched on the grid (tiles_x, n_cams, tiles_y) and reads its 16 x 16 pixel tile and its camera from
blockIdx: blocks run x fastest, then the camera, then the tile row, so that tile row r of every camera is dispatched before
row r + 1 of any.  Whatever the order, every ray of every camera must be rendered exactly once, by
the lane of the 8 x 8 wave that holds it in the camera-by-camera order: the skip decisions are wave-wide, so another tiling
changes the last bits, and a camera taken for a row (or the reverse) renders some rays twice and others never.

Lattices with ny in {1, 15, 16, 17, 33, 48, 49} and nx in {16, 37}: tiles_y = 1, 2, 3 and 4 with ragged last rows (and a
ragged last column), 1 and 3 cameras (n_cams below, equal to and above tiles_y), S in {9, 33}, inv_s in {20, 200}, face-safe
cell selection on and off (the two kernel instances).  The outputs are pre-filled with NaN through ``outputs=``: a ray that
is never written stays NaN.  Reference: ``ahead=False`` (so_march_fast, the step-by-step route on the linear block order);
all five outputs torch.equal.  Explicit rays of the same lattices (the linear launch) are the control.

Every launch takes the brick path (render.py: n_rays * S >= 16 * cells): the 6 x 5 x 4 volume of the phase test where the
lattice is large enough for it, else a 2 x 2 x 2 volume (one cell).
"""
import functools
import math

import numpy as np
import pytest
import torch

from selfocc_amd import synthetic as sy
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import render_rays, RaySet, RenderConfig, SDFVolume

KEYS = ("depth", "acc", "max_depth", "nears", "fars")
AABB = (0.0, 0.0, -1.0, 1.6, 2.0, 0.2)
NY_LIST, NX_LIST = (1, 15, 16, 17, 33, 48, 49), (16, 37)
# inside the box looking along it, inside looking back and down, outside looking in
POSES = (((0.3, 1.0, -0.3), 10.0, -6.0), ((1.2, 0.4, -0.2), 120.0, -10.0), ((-2.0, 1.0, -0.3), 5.0, -3.0))


def _mapping(h, w, d):
    return GridMeterMapping(nonlinear_mode='linear', h_size=[h - 1, 0], h_range=[2.0, 0], h_half=True, w_size=[w - 1, 0],
                            w_range=[1.6, 0], w_half=True, d_size=[d - 1, 0], d_range=[-1.0, 0.2, 0.2])


@functools.lru_cache(maxsize=None)
def volume(kind):
    """'tiny': 6 x 5 x 4 cells, a noisy floor under free space; 'cell': 2 x 2 x 2, the smallest volume there is"""
    m = _mapping(6, 5, 4) if kind == "tiny" else _mapping(2, 2, 2)
    z = sy.grid_points_meter(m)[..., 2]
    sdf = z + 0.75 + 0.02 * torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
    return SDFVolume(m, sdf.contiguous().float())


def camera(pos, yaw_deg, pitch_deg, nx, ny):
    """img2lidar of a pinhole at `pos` looking along (yaw, pitch), principal point at the lattice's centre"""
    yaw, pitch = math.radians(yaw_deg), math.radians(pitch_deg)
    fwd = np.array([math.cos(yaw) * math.cos(pitch), math.sin(yaw) * math.cos(pitch), math.sin(pitch)])
    right = np.array([math.sin(yaw), -math.cos(yaw), 0.0])
    down = np.cross(fwd, right)
    focal = 0.6 * max(nx, ny)
    K = np.array([[focal, 0, nx / 2.0, 0], [0, focal, ny / 2.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([right, down, fwd], axis=1)
    c2w[:3, 3] = pos
    return c2w @ np.linalg.inv(K)


def lattice(nx, ny, n_cams):
    mats = np.stack([camera(pos, yaw, pitch, nx, ny) for pos, yaw, pitch in POSES[:n_cams]])
    return RaySet(img2lidar=torch.tensor(mats, dtype=torch.float32), nx=nx, ny=ny, sx=1.0, sy=1.0)


def _render(vol, rays, S, inv_s, face_safe, ahead):
    """the five outputs of a launch into NaN-filled arrays"""
    out = {k: torch.full((rays.n_rays,), float("nan"), dtype=torch.float32, device=vol.sdf.device) for k in KEYS}
    got = render_rays(vol, rays, RenderConfig(aabb=AABB, n_samples=S, inv_s=inv_s, face_safe=face_safe, ahead=ahead), outputs=out)
    torch.cuda.synchronize()
    assert all(got[k] is out[k] for k in KEYS)
    return out


def _check(nx, ny, n_cams, S, mode):
    d = torch.device("cuda:0")
    rays = lattice(nx, ny, n_cams)
    kind = "tiny" if rays.n_rays * S >= 16 * volume("tiny").sdf.numel() else "cell"
    vol = volume(kind).to(d)
    assert rays.n_rays * S >= 16 * vol.sdf.numel(), "the launch must take the brick path"
    if mode == "explicit":
        e = sy.explicit_rays(rays)
        rays = RaySet(origins=e.origins.to(d), dirs=e.dirs.to(d), dir_norm=e.dir_norm.to(d))
    else:
        rays = RaySet(img2lidar=rays.img2lidar.to(d), nx=nx, ny=ny, sx=1.0, sy=1.0)
    hit = 0
    for inv_s in (20.0, 200.0):
        for face_safe in (True, False):
            run = _render(vol, rays, S, inv_s, face_safe, True)
            ref = _render(vol, rays, S, inv_s, face_safe, False)
            case = (nx, ny, n_cams, S, mode, kind, inv_s, face_safe)
            for k in KEYS:
                n_nan = int(torch.isnan(run[k]).sum())
                assert n_nan == 0, (case, k, f"{n_nan} rays were never written")
                assert not torch.isnan(ref[k]).any(), (case, k)
                assert torch.equal(run[k], ref[k]), (case, k, int((run[k] != ref[k]).sum()))
            hit += int((run["acc"] > 0.5).sum())
    print(f"[row-order] {mode} nx={nx} ny={ny} cams={n_cams} S={S} volume={kind}: rays {rays.n_rays}, "
          f"tiles_y={(ny + 15) // 16}, rays with acc > 0.5 over the four launches: {hit}")
    return hit


@pytest.mark.gpu
@pytest.mark.parametrize("S", [9, 33])
@pytest.mark.parametrize("n_cams", [1, 3])
@pytest.mark.parametrize("nx", NX_LIST)
@pytest.mark.parametrize("ny", NY_LIST)
def test_every_ray_once_pixel_grid(hip, ny, nx, n_cams, S):
    _check(nx, ny, n_cams, S, "pixgrid")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [9, 33])
@pytest.mark.parametrize("n_cams", [1, 3])
@pytest.mark.parametrize("nx", NX_LIST)
@pytest.mark.parametrize("ny", NY_LIST)
def test_explicit_rays_control(hip, ny, nx, n_cams, S):
    """the same lattices as explicit rays: the launch that keeps its linear order"""
    _check(nx, ny, n_cams, S, "explicit")
