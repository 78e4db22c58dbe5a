"""GPU: the near-face block of the code-ahead skip marcher (csrc/render_fwd.hip, so_march_fast_ahead).

A sample whose affine grid coordinate lies within face_m of a voxel face may fall into the neighbouring cell under the
canonical operation order, so a wave with such a lane leaves the step's straight path: the lane re-derives its sample in
the canonical order (its unit direction comes back from the lane's LDS slot, parked there before the march), takes the
canonical cell when that is another one, and the wave then gathers its corners from the volume instead of the brick.
The block is rare in a real frame (under 2 % of the interpolated wave-steps), so these scenes force it: a camera looks
along a grid axis from a position that puts one grid coordinate of the centre column (or row) of the lattice at
integer + k float32 steps for the whole ray, k = -3 .. 3, on each of the three axes, plus one placement with two axes
at a face at once.

Reference: ``ahead=False, face_safe=True`` (so_march_fast, an independent route through the same library); all five
outputs torch.equal, on pixel-grid and on explicit rays, S in {33, 64}, inv_s in {20, 200}.

Conditions on the inputs (not on the code under test), so that no case is vacuous:
  * the affine coordinates are rebuilt on the CPU (the fma as a float64 product and sum rounded once to float32) and the
    wave-steps with a near-face lane are counted: every placement has MIN_NEAR_WAVE_STEPS of them or more;
  * on each axis at least 2 of the 7 placements give bitwise different outputs between face_safe=True and
    face_safe=False on the ``ahead=False`` route: a lane really moved to the neighbouring cell, so the gather rejoin runs.
"""
import functools
import math

import numpy as np
import pytest
import torch

from selfocc_amd import synthetic as sy
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import render_rays, RaySet, RenderConfig, SDFVolume

pytestmark = pytest.mark.gpu

KEYS = ("depth", "acc", "max_depth", "nears", "fars")
NX, NY, FOCAL = 24, 16, 16.0                     # centre column ix = 12, centre row iy = 8; 1 / FOCAL is a power of two
AABB = (0.0, 0.0, -1.0, 4.4, 5.2, 1.2)           # x <-> w (10 points), y <-> h (12), z <-> d (6); no cell size is a binary fraction
S_LIST, INV_S_LIST, MODES = (33, 64), (20.0, 200.0), ("pixgrid", "explicit")
KS = (0, 1, -1, 2, -2, 3, -3)
FACE_Y, FACE_X, FACE_Z = 7 * 5.2 / 11, 2 * 4.4 / 9, -1.0 + 2 * 2.2 / 5        # h = 7, w = 2, d = 2
f32 = np.float32


def mapping():
    return GridMeterMapping(nonlinear_mode='linear', h_size=[11, 0], h_range=[5.2, 0], h_half=True, w_size=[9, 0],
                            w_range=[4.4, 0], w_half=True, d_size=[5, 0], d_range=[-1.0, 1.2, 1.2])


@functools.lru_cache(maxsize=None)
def volume():
    """12 x 10 x 6 cells, synthetic.make_volume's recipe: a ground plane, boxes, noise"""
    m = mapping()
    xyz = sy.grid_points_meter(m)
    gen = torch.Generator().manual_seed(5)
    sdf = xyz[..., 2] + 0.2
    for c, half in (((2.6, 3.2, 0.1), (0.4, 0.5, 0.5)), ((1.1, 4.0, 0.3), (0.5, 0.4, 0.7)), ((3.6, 1.2, 0.0), (0.4, 0.4, 0.4))):
        q = (xyz - torch.tensor(c)).abs() - torch.tensor(half)
        sdf = torch.minimum(sdf, torch.linalg.norm(q.clamp_min(0.0), dim=-1) + q.max(dim=-1).values.clamp_max(0.0))
    sdf = sdf + 0.05 * torch.randn(sdf.shape, generator=gen)
    assert tuple(sdf.shape) == (12, 10, 6)
    return SDFVolume(m, sdf.contiguous().float())


def steps(x, k):
    """x moved by k float32 steps"""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return float(x)


def camera(pos, yaw_deg):
    """img2lidar of a level pinhole at `pos` looking along yaw (synthetic.make_cameras' convention).  At yaw 0 / 90 the
    centre column of the lattice has a direction with y / x exactly 0, the centre row one with z exactly 0."""
    yaw = math.radians(yaw_deg)
    fwd = np.array([math.cos(yaw), math.sin(yaw), 0.0])
    right = np.array([math.sin(yaw), -math.cos(yaw), 0.0])
    down = np.array([0.0, 0.0, -1.0])
    K = np.array([[FOCAL, 0, NX / 2.0, 0], [0, FOCAL, NY / 2.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([right, down, fwd], axis=1)
    c2w[:3, 3] = pos
    return c2w @ np.linalg.inv(K)


def placements():
    """name -> (axis or None, camera): the grid coordinate of the named axis at integer + k float32 steps of the metre value.
    The faces are ones at which the canonical order and the affine form round to different sides for some of the k (with
    cell sizes that are binary fractions they never do)."""
    p = {}
    for k in KS:
        p[f"h{k:+d}"] = ("h", camera((0.25, steps(FACE_Y, k), 0.3), 0.0))
        p[f"w{k:+d}"] = ("w", camera((steps(FACE_X, k), 0.25, 0.3), 90.0))
        p[f"d{k:+d}"] = ("d", camera((0.25, 2.7, steps(FACE_Z, k)), 0.0))
    p["h+0_d+1"] = (None, camera((0.25, steps(FACE_Y, 0), steps(FACE_Z, 1)), 0.0))
    return p


PLACEMENTS = placements()
assert len(PLACEMENTS) == 22


def lattice(cam):
    return RaySet(img2lidar=torch.tensor(cam[None], dtype=torch.float32), nx=NX, ny=NY, sx=1.0, sy=1.0)


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def near_face_wave_steps(cam, S, mode):
    """wave-steps at which some lane's affine grid coordinate (so_march_fast_ahead's `place`) is within face_m of a voxel
    face, and the number of waves.  A wave is an 8 x 8 pixel tile (pixel grid) or 64 consecutive rays (explicit)."""
    r = sy.explicit_rays(lattice(cam))
    o, d = r.origins.numpy().astype(f32), r.dirs.numpy().astype(f32)
    lo, hi = np.array(AABB[:3], f32), np.array(AABB[3:], f32)
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = f32(1.0) / (d + f32(1e-6))
        ta, tb = (lo - o) * inv, (hi - o) * inv
    tnear = np.maximum(np.minimum(ta, tb).max(1), f32(0.0))
    tfar = np.maximum(np.maximum(ta, tb).min(1), tnear + f32(1e-6))
    dt = (tfar - tnear) / f32(S)
    m = mapping().to_abi()
    near = np.zeros((o.shape[0], S), bool)
    maxdim = max(m.h.tot_len, m.w.tot_len, m.d.tot_len)
    face_m = f32(3.0) * f32(1.1920929e-7) * f32(1 << maxdim.bit_length())
    for ax, col in ((m.h, 1), (m.w, 0), (m.d, 2)):
        k1 = f32(ax.size0) / f32(ax.range0)
        k0 = (f32(ax.off0) + f32(ax.off1)) - f32(ax.start) * k1
        Gd = d[:, col] * k1
        G0 = fma32(o[:, col], np.full_like(Gd, k1), np.full_like(Gd, k0)) + Gd * tnear
        step = np.arange(S, dtype=f32)[None, :] * dt[:, None]
        g = fma32(np.broadcast_to(Gd[:, None], step.shape), step, np.broadcast_to(G0[:, None], step.shape))
        fr = g - np.floor(g)
        near |= np.abs(fr - f32(0.5)) > f32(0.5) - face_m
    if mode == "pixgrid":
        waves = near.reshape(NY // 8, 8, NX // 8, 8, S).transpose(0, 2, 1, 3, 4).reshape(-1, 64, S)
    else:
        waves = near.reshape(-1, 64, S)
    return int(waves.any(1).sum()), waves.shape[0]


@functools.lru_cache(maxsize=None)
def _render(name, S, inv_s, mode, ahead, face_safe):
    d = torch.device("cuda:0")
    rays = lattice(PLACEMENTS[name][1])
    if mode == "explicit":
        e = sy.explicit_rays(rays)
        rays = RaySet(origins=e.origins.to(d), dirs=e.dirs.to(d), dir_norm=e.dir_norm.to(d))
    else:
        rays = RaySet(img2lidar=rays.img2lidar.to(d), nx=NX, ny=NY, sx=1.0, sy=1.0)
    vol = volume().to(d)
    assert rays.n_rays * S >= 16 * vol.sdf.numel(), "the launch must take the brick path"
    out = render_rays(vol, rays, RenderConfig(aabb=AABB, n_samples=S, inv_s=inv_s, ahead=ahead, face_safe=face_safe))
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in KEYS}


def _differ(a, b):
    return sum(int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum()) for k in KEYS)


# Lower bounds, a little under what the CPU count gives (the smallest over the 22 placements is 70 / 134 wave-steps on the
# pixel grid and 41 / 71 on explicit rays, at S = 33 / 64, of 6 waves x S): the centre column or row sits at a face for the
# whole march, and 2 or 3 of the 6 waves hold a part of it.
MIN_NEAR_WAVE_STEPS = {("pixgrid", 33): 60, ("pixgrid", 64): 120, ("explicit", 33): 35, ("explicit", 64): 60}
# Placements per axis whose outputs canonical cell selection changes, as observed on the step-by-step route on MI355X, in
# all 8 combinations of S, inv_s and ray mode: k = 0, -1 on h (722 - 731 differing output values at inv_s 20, 5 - 8 at 200),
# k = 0, +1 on w (326 - 330 and 4 - 10) and every k but -3 on d (579 - 601 and 455 - 458).  A CPU restatement of the canonical
# order predicts exactly these.
MIN_MOVED_PLACEMENTS = {"h": 2, "w": 2, "d": 6}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("inv_s", INV_S_LIST)
@pytest.mark.parametrize("S", S_LIST)
@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_near_face_block_equals_step_by_step(hip, name, S, inv_s, mode):
    n_near, n_waves = near_face_wave_steps(PLACEMENTS[name][1], S, mode)
    run = _render(name, S, inv_s, mode, True, True)
    ref = _render(name, S, inv_s, mode, False, True)
    bad = {k: int((run[k].view(torch.int32) != ref[k].view(torch.int32)).sum()) for k in KEYS}
    print(f"[face-cold] {name} S={S} inv_s={inv_s} {mode}: near-face wave-steps={n_near} of {n_waves * S}; differing values {bad}")
    assert n_near >= MIN_NEAR_WAVE_STEPS[(mode, S)], (name, n_near)
    for k in KEYS:
        assert torch.equal(run[k], ref[k]), (name, S, inv_s, mode, k, bad[k])
    assert torch.isfinite(run["depth"]).all() and torch.isfinite(run["acc"]).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("inv_s", INV_S_LIST)
@pytest.mark.parametrize("S", S_LIST)
@pytest.mark.parametrize("axis", ["h", "w", "d"])
def test_placements_move_lanes(hip, axis, S, inv_s, mode):
    """the inputs, on the reference route alone: canonical cell selection changes the outputs of at least 2 placements of the axis"""
    moved = {}
    for name, (ax, _) in PLACEMENTS.items():
        if ax == axis:
            moved[name] = _differ(_render(name, S, inv_s, mode, False, True), _render(name, S, inv_s, mode, False, False))
    n = sum(v > 0 for v in moved.values())
    print(f"[face-cold] axis {axis} S={S} inv_s={inv_s} {mode}: values that face_safe changes, per placement: {moved}; placements: {n}")
    assert n >= MIN_MOVED_PLACEMENTS[axis], (axis, moved)
