"""GPU: interpolated stretches of the code-ahead skip marcher (csrc/render_fwd.hip, so_march_fast_ahead, sure loop).

Inside a stretch of interpolated ("full") steps that hugs a surface, most wave-steps hold a lane whose cell has a corner
under the saturation level 17.5 / inv_s.  The brick pass gives such a cell the skip code 0 (`slack > 0` fails), so the wave
cannot skip and the code byte it loads for the step can only say so.  A marcher may use that — decide a step from the
corners it loads anyway and leave the code load out — and whatever it does there must not change a bit of the outputs.
These scenes put every transition of such a scheme in front of the kernel:

  * floor: a level camera grazes a floor, long stretches of full steps that some lane's corners prove unskippable, ending in
    free space (proven ... -> not proven -> skipped -> free-space run) or at the end of the sure range (S from 9 to 128); in
    that free space the SDF falls along the rays, so interpolating a step that should have been skipped changes output bits;
  * ramp: cells whose corners all exceed 17.5 / inv_s but whose code is below the ray's (a steep gradient, long dt): not
    provable from the corners, and not skipped either;
  * boundary: inv_s = 17.5, so the saturation level is exactly 1.0f, with corners exactly 1.0f, 1.0f +- 1 ulp and
    1.0f +- 8 ulp in the cells the rays cross: `>` against `>=`, or a threshold off by a rounding, decide differently here;
  * near a face: the placements of tests/test_render_face_cold_gpu.py (a grid coordinate held at integer + k float32 steps)
    over the floor, so that the near-face steps fall inside a provable stretch;
  * the slab of tests/test_render_skip_run_gpu.py.

Reference: ``ahead=False`` (so_march_fast), an independent route through the same library that decides and composites
every step on its own; all five outputs torch.equal.  Every launch is given the brick workspace (as in
tests/test_render_launch_consts_gpu.py), so every case takes the skip marcher.

No case is vacuous: `wave_counts` restates the march on the CPU (float32 numpy: the affine grid coordinates, the brick
pass's skip codes, the wave-wide decisions, corner v0 against the threshold, the near-face test, the exit test) and walks every wave through the step kinds; each case asserts the kinds it is meant to reach.  The arithmetic of
the restatement follows the kernel's, but only its counts are used, never its values.  scripts/skip_low_mode_stats.py
prints the same counts for the benchmark frame.
"""
import collections
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from selfocc_amd import synthetic as sy
from selfocc_amd._lib import check, current_stream, lib, ptr
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import RaySet, RenderConfig, SDFVolume, _brick_workspace, marshal_render_args

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_skip_run_scenes", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  "test_render_skip_run_gpu.py"))
_sr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_sr)

KEYS = ("depth", "acc", "max_depth", "nears", "fars")
f32, f64 = np.float32, np.float64
AABB = (0.0, 0.0, -1.0, 4.4, 5.2, 1.2)           # x <-> w (10 points), y <-> h (12), z <-> d (6): the face-cold volume's box
FOCAL = 16.0
LOG2E = f32(1.44269504088896341)
# A step is "provable" when some lane's corner v0 (the cell's own grid point) is at or under LOW_C / s2, s2 = fl(inv_s * log2 e):
# LOW_C lies 15 * 2^-24 relative below 17.5 * log2 e, so the roundings of s2, of the reciprocal and of the product cannot make a
# cell provable that the brick pass (smallest corner > fl(17.5 / inv_s)) gives a non-zero code.
LOW_C = f32(25.24714)
K_ALPHA_FREE = f32(1e-5) / (f32(1.0) + f32(1e-5))
K_SURE_SCAN = 8
ENTER_AFTER = 2          # sure steps in a row in which no lane could skip (the hint) before the mode opens


def mapping():
    return GridMeterMapping(nonlinear_mode='linear', h_size=[11, 0], h_range=[5.2, 0], h_half=True, w_size=[9, 0],
                            w_range=[4.4, 0], w_half=True, d_size=[5, 0], d_range=[-1.0, 1.2, 1.2])


def camera(pos, yaw_deg, pitch_deg, nx, ny):
    """img2lidar of a pinhole at `pos` looking along (yaw, pitch) (synthetic.make_cameras' convention)"""
    yaw, pitch = math.radians(yaw_deg), math.radians(pitch_deg)
    fwd = np.array([math.cos(yaw) * math.cos(pitch), math.sin(yaw) * math.cos(pitch), math.sin(pitch)])
    right = np.array([math.sin(yaw), -math.cos(yaw), 0.0])
    down = np.cross(fwd, right)
    K = np.array([[FOCAL, 0, nx / 2.0, 0], [0, FOCAL, ny / 2.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    c2w = np.eye(4)
    c2w[:3, :3] = np.stack([right, down, fwd], axis=1)
    c2w[:3, 3] = pos
    return c2w @ np.linalg.inv(K)


# the first camera is level and grazes the floor; the others look a little up and down from other corners
POSES = (((0.15, 2.7, -0.86), 0.0, 0.0), ((0.3, 0.4, -0.55), 50.0, 9.0), ((4.2, 4.9, -0.3), 228.0, -4.0))


def lattice(nx, ny, n_cams, poses=POSES):
    mats = np.stack([camera(pos, yaw, pitch, nx, ny) for pos, yaw, pitch in poses[:n_cams]])
    return RaySet(img2lidar=torch.tensor(mats, dtype=torch.float32), nx=nx, ny=ny, sx=1.0, sy=1.0)


def _noise(seed):
    return torch.randn((12, 10, 6), generator=torch.Generator().manual_seed(seed))


def steps_f32(x, k):
    """x moved by k float32 steps"""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


@functools.lru_cache(maxsize=None)
def scene_sdf(kind):
    xyz = sy.grid_points_meter(mapping())
    x, z = xyz[..., 0], xyz[..., 2]
    if kind in ("floor", "floor200"):
        # A floor at z = -0.9 that ends in a cliff at x = 2.9.  Behind it the SDF stands a little above the saturation level
        # L (0.875 m at inv_s 20, 0.0875 m at 200) and FALLS along x: free space in which the rays' cosine is negative and the
        # sigmoid arguments stay under ~35, so an interpolated step there composites an alpha a few 1e-11 off the constant
        # one of a skipped step — a marcher that interpolates a step it should have skipped changes output bits.
        L = 0.875 if kind == "floor" else 0.0875
        floor = (z + 0.9) + 0.01 * _noise(3)
        beyond = L * (1.4 - 0.1 * (x - 2.9)) + 0.002 * L * _noise(6)
        sdf = torch.where(x > 2.9, beyond, floor)
    elif kind in ("ramp", "ramp200"):
        # Planes of constant value along x, in units of the saturation level L (0.875 m at inv_s 20, 0.0875 m at 200): under
        # the level at the first plane, then a steep rise — the cells between the second and third plane have every corner
        # above the level, by so little against their gradient that their code stays under the ray's — then a fall in free
        # space, where a marcher that went on interpolating would composite other bits than one that skips.
        L = 0.875 if kind == "ramp" else 0.0875
        col = torch.tensor([0.3, 1.066, 1.9, 1.4, 1.35, 1.3, 1.25, 1.2, 1.15, 1.1])
        sdf = L * (col[None, :, None].expand(12, 10, 6) + 0.002 * _noise(4))
    elif kind == "boundary":
        # planes of constant value along x (w): a low region the marcher starts in, then corners at the level 1.0f itself;
        # the values change along x only, so cells between two planes above the level have a tiny gradient and a large code
        one = f32(1.0)
        col = [0.4, 0.5, steps_f32(one, 8), steps_f32(one, 8), steps_f32(one, 1), one, steps_f32(one, -1), steps_f32(one, -8),
               1.4, 1.3]         # the last two: free space in which the SDF falls along x, as in the floor scene
        sdf = torch.tensor(np.array(col, dtype=f32))[None, :, None].expand(12, 10, 6).clone()
        sdf[:, :, 4:] = 3.0          # and a ceiling of plain free space above it
    else:
        raise KeyError(kind)
    assert tuple(sdf.shape) == (12, 10, 6)
    return sdf.contiguous().float()


def volume(kind):
    return SDFVolume(mapping(), scene_sdf(kind))


# ---- the launch -------------------------------------------------------------------------------------------------------
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


def both_routes(vol, rays, mode, aabb, S, inv_s, how="value", face_safe=True):
    d = torch.device("cuda:0")
    r = on_gpu(sy.explicit_rays(rays) if mode == "explicit" else rays)
    dvol = vol.to(d)
    ref = launch(dvol, r, RenderConfig(aabb=aabb, n_samples=S, inv_s=inv_s, ahead=False, face_safe=face_safe))
    if how == "device":     # the kernels must read the device's value: the host field holds another one
        cfg = RenderConfig(aabb=aabb, n_samples=S, inv_s=0.5 * inv_s, face_safe=face_safe,
                           inv_s_dev=torch.tensor([inv_s], dtype=torch.float32, device=d))
    else:
        cfg = RenderConfig(aabb=aabb, n_samples=S, inv_s=inv_s, face_safe=face_safe)
    return launch(dvol, r, cfg), ref


def assert_equal(got, ref, case):
    bad = {k: int((got[k].view(torch.int32) != ref[k].view(torch.int32)).sum()) for k in KEYS}
    print(f"[low-mode] {case}: rays {ref['acc'].numel()}; differing values {bad}")
    for k in KEYS:
        assert torch.equal(got[k], ref[k]), (case, k, bad[k])


# ---- the march, restated on the CPU -------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def wave_lanes(rays, mode):
    """(n_waves, 64) ray indices of every wave, -1 for a lane without a ray: an 8 x 8 pixel tile of one camera (pixel grid)
    or 64 consecutive rays (explicit)"""
    n_cams, nx, ny = rays.img2lidar.shape[0], rays.nx, rays.ny
    if mode == "explicit":
        n = n_cams * nx * ny
        idx = np.full(((n + 63) // 64) * 64, -1, np.int64)
        idx[:n] = np.arange(n)
        return idx.reshape(-1, 64)
    tx, ty = (nx + 7) // 8, (ny + 7) // 8
    ix = np.arange(tx * 8)[None, :].repeat(ty * 8, 0)
    iy = np.arange(ty * 8)[:, None].repeat(tx * 8, 1)
    per_cam = np.where((ix < nx) & (iy < ny), iy * nx + ix, -1)
    tiles = per_cam.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    out = [np.where(tiles >= 0, tiles + c * nx * ny, -1) for c in range(n_cams)]
    return np.concatenate(out, 0)


def wave_tables(sdf, codes, mapping_abi, aabb, S, inv_s, o, d, lanes, corner_forms=False):
    """Per wave and step, the wave-wide facts the marcher decides on.  o, d: (N, 3) float32 origins and unit directions;
    lanes: (n_waves, 64) ray indices (wave_lanes).  Returns a dict of (n_waves, S) bool arrays — `interior`, `free` (all
    lanes' codes reach the ray's), `provable`, `hint`, `near`, `exit` (after the step, with the skip decisions of the
    parent), `marched` (the march reaches the step) — and the sure range (i_lo, i_hi) of every wave.  corner_forms: also
    `provable_8` / `provable_2`, the predicate on the 8-corner minimum / on min(v0, v7), and `sdf_low`: some lane's
    interpolated sdf * s2 <= LOW_C."""
    H, W, D = sdf.shape
    valid = lanes >= 0
    li = np.where(valid, lanes, 0)
    o, d = o[li], d[li]                                              # (Wv, 64, 3)
    lo, hi = np.array(aabb[:3], f32), np.array(aabb[3:], f32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        inv = f32(1.0) / (d + f32(1e-6))
        ta, tb = (lo - o) * inv, (hi - o) * inv
        tnear = np.maximum(np.minimum(ta, tb).max(-1), f32(0.0))
        tfar = np.maximum(np.maximum(ta, tb).min(-1), tnear + f32(1e-6))
        dt = (tfar - tnear) / f32(S)
        maxdim = max(H, W, D)
        face_m = f32(3.0) * f32(1.1920929e-7) * f32(1 << maxdim.bit_length())
        fi = np.arange(S, dtype=f32)
        step = fi[None, None, :] * dt[..., None]                      # (Wv, 64, S)
        g, Gd = [], []
        for ax, col in ((mapping_abi.h, 1), (mapping_abi.w, 0), (mapping_abi.d, 2)):
            k1 = f32(ax.size0) / f32(ax.range0)
            k0 = (f32(ax.off0) + f32(ax.off1)) - f32(ax.start) * k1
            gd_ = d[..., col] * k1
            g0 = fma32(o[..., col], np.full_like(gd_, k1), np.full_like(gd_, k0)) + gd_ * tnear
            g.append(fma32(np.broadcast_to(gd_[..., None], step.shape), step, np.broadcast_to(g0[..., None], step.shape)))
            Gd.append(gd_)
        c0 = [np.floor(x) for x in g]
        fr = [x - c for x, c in zip(g, c0)]
        ci = [np.nan_to_num(c, nan=-1.0, posinf=-1.0, neginf=-1.0).astype(np.int64) for c in c0]
        inside = (ci[0] >= 0) & (ci[0] < H - 1) & (ci[1] >= 0) & (ci[1] < W - 1) & (ci[2] >= 0) & (ci[2] < D - 1)
        vmask = valid[..., None]
        interior = (inside | ~vmask).all(1)
        h0, w0, d0 = (np.clip(c, 0, n - 2) for c, n in zip(ci, (H, W, D)))
        ex, ey, ez = f32(aabb[3]) - f32(aabb[0]), f32(aabb[4]) - f32(aabb[1]), f32(aabb[5]) - f32(aabb[2])
        unit = np.sqrt(ex * ex + ey * ey + ez * ez) / (f32(float(S)) * f32(255.0))
        rcode = np.maximum(np.ceil(dt / unit), f32(1.0))
        lane_free = codes[h0, w0, d0].astype(f32) >= rcode[..., None]
        free = interior & (lane_free | ~vmask).all(1)
        v = [sdf[h0 + a, w0 + b, d0 + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)]     # v0 .. v7 of the brick pass
        m = functools.reduce(np.fmin, v)
        s2 = f32(inv_s) * LOG2E
        thr = LOW_C * (f32(1.0) / s2)
        provable = ((v[0] <= thr) & vmask).any(1)
        near = ((np.maximum(np.maximum(np.abs(fr[0] - f32(0.5)), np.abs(fr[1] - f32(0.5))), np.abs(fr[2] - f32(0.5))) > f32(0.5) - face_m) & vmask).any(1)
        # the interpolation and alpha of so_trilerp_fast_pk / so_alpha_fast (for the hint and the transmittance)
        fh, fw, fd = fr
        c = [fma32(fd, v[2 * k + 1] - v[2 * k], v[2 * k]) for k in range(4)]
        dw0, dw1 = c[1] - c[0], c[3] - c[2]
        b0, b1 = fma32(fw, dw0, c[0]), fma32(fw, dw1, c[2])
        gvh = b1 - b0
        val = fma32(fh, gvh, b0)
        gvw = fma32(fh, dw1 - dw0, dw0)
        dd = [v[2 * k + 1] - v[2 * k] for k in range(4)]
        e0, e1 = fma32(fw, dd[1] - dd[0], dd[0]), fma32(fw, dd[3] - dd[2], dd[2])
        gvd = fma32(fh, e1 - e0, e0)
        cosv = fma32(gvd, Gd[2][..., None], fma32(gvw, Gd[1][..., None], gvh * Gd[0][..., None]))
        xs = val * s2
        hs = np.minimum(cosv, f32(0.0)) * (f32(0.5) * dt * s2)[..., None]
        ea, eb = np.exp2(np.minimum(hs - xs, f32(60.0))), np.exp2(np.minimum(-hs - xs, f32(60.0)))
        p = f32(1.0) + ea
        alpha = np.minimum(fma32(eb - ea, f32(1.0) / (f32(1.0) + eb), f32(1e-5) * p) / fma32(np.full_like(p, f32(1e-5)), p, np.ones_like(p)), f32(1.0))
        hint = (~lane_free | ~vmask).all(1)                            # no lane's code reaches its ray's
        T = np.ones(lanes.shape, f32)
        exit_ = np.zeros(free.shape, bool)
        for i in range(S):
            a_i = np.where(free[:, None, i], K_ALPHA_FREE, alpha[..., i]).astype(f32)
            T = T * ((f32(1.0) - a_i) + f32(1e-7))
            exit_[:, i] = ((T < f32(1e-10)) | ~valid).all(1)
    marched = np.concatenate([np.ones((lanes.shape[0], 1), bool), np.cumsum(exit_[:, :-1], 1) == 0], 1)
    tab = dict(interior=interior, free=free, provable=provable, hint=hint, near=near, exit=exit_, marched=marched)
    if corner_forms:
        tab["provable_8"] = ((m <= thr) & vmask).any(1)
        tab["provable_2"] = ((np.fmin(v[0], v[7]) <= thr) & vmask).any(1)
        tab["sdf_low"] = ((xs <= LOW_C) & vmask).any(1)
    n = min(K_SURE_SCAN, S)
    i_lo, i_hi = np.full(lanes.shape[0], S), np.full(lanes.shape[0], -1)
    for w in range(lanes.shape[0]):
        first = np.flatnonzero(interior[w, :n])
        if first.size:
            last = [k for k in range(S - 1, max(S - n, first[0]) - 1, -1) if interior[w, k]]
            if last:
                i_lo[w], i_hi[w] = first[0], last[0]
    return tab, i_lo, i_hi


def walk_wave(S, i_lo, i_hi, t, w, face_safe=True, enter_after=ENTER_AFTER):
    """One wave through the phases of so_march_fast_ahead.  Counts: full / skip steps of the march itself; stretch starts;
    for a marcher that leaves the code load out of proven steps inside full-step stretches (entered behind the second step
    of the sure loop's body after `enter_after` steps in a row whose hint held; a near-face step, an unproven step or the
    range's end leaves): steps proven,
    unproven and kept, unproven and skipped, near-face exits; vector-memory instructions with and without that mode."""
    c = collections.Counter()
    free, prov, hint, near, exit_ = t["free"][w], t["provable"][w], t["hint"][w], t["near"][w], t["exit"][w]
    state = dict(prev_full=False, hinted=0)      # hinted: interpolated sure steps in a row whose hint held

    def step(i, sk, code_load=True):          # a step of the parent: one code load for the next step, two record loads if full
        c["skip" if sk else "full"] += 1
        if not sk and not state["prev_full"]:
            c["stretch_starts"] += 1
        if not sk and prov[i]:
            c["full_provable"] += 1
        state["prev_full"] = not sk
        n = (1 if (code_load and i + 1 < S) else 0) + (0 if sk else 2)
        c["vmem_parent"] += n
        return n

    i = 0
    while i < min(i_lo, S):                                   # head (or the whole march of a wave without a sure range)
        c["vmem_low"] += step(i, bool(free[i]))
        i += 1
        if i >= S or exit_[i - 1]:
            return c
    while i < i_hi:                                           # sure loop: the two halves of its body, then the mode's entry
        entered = False
        for half in (0, 1):
            sk = bool(free[i])
            c["vmem_low"] += step(i, sk)
            state["hinted"] = state["hinted"] + 1 if (not sk and hint[i]) else 0
            i += 1
            if exit_[i - 1]:
                return c
            while sk and i < i_hi and free[i]:                # run loop
                c["vmem_low"] += step(i, True)
                i += 1
                if exit_[i - 1]:
                    return c
            if i >= i_hi:
                break
            entered = half == 1 and state["hinted"] >= enter_after
        if entered:
            c["low_entries"] += 1
            while True:
                if i + 1 >= i_hi:
                    c["low_range_end"] += 1
                    c["vmem_low"] += 1
                    break
                if face_safe and near[i]:
                    c["low_near_face"] += 1
                    c["vmem_low"] += 1
                    break
                if prov[i]:
                    c["low_proven"] += 1
                    step(i, False, code_load=False)
                    c["vmem_parent"] += 1
                    c["vmem_low"] += 2
                    i += 1
                    if exit_[i - 1]:
                        return c
                    continue
                sk = bool(free[i])
                c["low_unproven_skipped" if sk else "low_unproven_kept"] += 1
                step(i, sk, code_load=False)
                c["vmem_parent"] += 1
                c["vmem_low"] += 4
                i += 1
                if exit_[i - 1]:
                    return c
                break
    while i < S:                                              # tail
        c["vmem_low"] += step(i, bool(free[i]))
        i += 1
        if i < S and exit_[i - 1]:
            return c
    return c


def wave_counts(sdf_t, mapping_, aabb, S, inv_s, rays, mode, face_safe=True):
    """the counts of walk_wave summed over the waves of a launch, plus `waves`"""
    codes, _ = _sr.skip_codes_torch(sdf_t, mapping_, aabb, S, inv_s)
    e = sy.explicit_rays(rays)
    lanes = wave_lanes(rays, mode)
    t, i_lo, i_hi = wave_tables(sdf_t.numpy(), codes.numpy(), mapping_.to_abi(), aabb, S, inv_s, e.origins.numpy().astype(f32),
                                e.dirs.numpy().astype(f32), lanes)
    total = collections.Counter(waves=lanes.shape[0])
    for w in range(lanes.shape[0]):
        total.update(walk_wave(S, int(i_lo[w]), int(i_hi[w]), t, w, face_safe))
    return total


def _show(case, n):
    print(f"[low-mode] {case}: " + ", ".join(f"{k}={n[k]}" for k in ("waves", "full", "skip", "full_provable", "stretch_starts",
          "low_entries", "low_proven", "low_unproven_kept", "low_unproven_skipped", "low_near_face", "low_range_end",
          "vmem_parent", "vmem_low")))


# ---- the cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ("value", "device"))
@pytest.mark.parametrize("inv_s", (20.0, 200.0))
@pytest.mark.parametrize("S", (9, 17, 33, 64, 128))
@pytest.mark.parametrize("mode", ("pixgrid", "explicit"))
@pytest.mark.parametrize("n_cams", (1, 3))
@pytest.mark.parametrize("nx,ny", ((24, 16), (37, 19)))
def test_floor_stretches(hip, nx, ny, n_cams, mode, S, inv_s, how):
    """long provable stretches over the floor that end in free space, in the cliff's shadow or at the end of the sure range"""
    rays = lattice(nx, ny, n_cams)
    case = ("floor", nx, ny, n_cams, mode, S, inv_s, how)
    kind = "floor" if inv_s == 20.0 else "floor200"
    n = wave_counts(scene_sdf(kind), mapping(), AABB, S, inv_s, rays, mode)
    _show(case, n)
    assert n["low_proven"] > 0 and (S < 17 or n["low_proven"] >= n["waves"]), (case, n)      # stretches, not single steps
    assert n["low_range_end"] > 0 or n["low_unproven_skipped"] > 0, (case, n)
    if S >= 33 and mode == "pixgrid":       # a stretch that ends in free space (8 x 8 tiles: the lanes leave the floor together)
        assert n["low_unproven_skipped"] > 0 and n["skip"] > 0, (case, n)
    got, ref = both_routes(volume(kind), rays, mode, AABB, S, inv_s, how)
    assert_equal(got, ref, case)


@pytest.mark.parametrize("mode", ("pixgrid", "explicit"))
@pytest.mark.parametrize("S", (9, 33, 64))
@pytest.mark.parametrize("kind,inv_s", (("ramp", 20.0), ("ramp200", 200.0)))
def test_unproven_and_not_skipped(hip, kind, inv_s, S, mode):
    """cells above the saturation level whose code is below the ray's: the corners prove nothing and the code says no"""
    rays = lattice(16, 33, 3)
    case = (kind, mode, S, inv_s)
    n = wave_counts(scene_sdf(kind), mapping(), AABB, S, inv_s, rays, mode)
    _show(case, n)
    assert n["low_unproven_kept"] > 0 and n["low_proven"] > 0, (case, n)
    got, ref = both_routes(volume(kind), rays, mode, AABB, S, inv_s)
    assert_equal(got, ref, case)


@pytest.mark.parametrize("mode", ("pixgrid", "explicit"))
@pytest.mark.parametrize("S", (17, 33, 64))
def test_saturation_boundary(hip, S, mode):
    """inv_s = 17.5: the level is 1.0f.  Rays cross planes of corners at 1.0f + 8, + 1, 0, - 1, - 8 ulp after a low region."""
    poses = (((0.1, 2.6, -0.4), 0.0, 0.0), ((0.2, 0.5, -0.6), 40.0, 3.0), ((0.1, 4.6, 0.1), -35.0, -3.0))
    rays = lattice(24, 16, 3, poses)
    case = ("boundary", mode, S)
    sdf = scene_sdf("boundary")
    codes, _ = _sr.skip_codes_torch(sdf, mapping(), AABB, S, 17.5)
    above = sdf[:, 2:8, :4] > 1.0
    assert int((codes[:, 2:8, :3] > 0).sum()) > 0 and int((codes[:, 2:8, :3] == 0).sum()) > 0     # the level cuts through these cells
    assert int(above.sum()) > 0 and int((~above).sum()) > 0
    n = wave_counts(sdf, mapping(), AABB, S, 17.5, rays, mode)
    _show(case, n)
    assert n["low_entries"] > 0 and n["low_unproven_kept"] + n["low_unproven_skipped"] > 0, (case, n)
    got, ref = both_routes(volume("boundary"), rays, mode, AABB, S, 17.5)
    assert_equal(got, ref, case)


FACE_Y, FACE_X, FACE_Z = 7 * 5.2 / 11, 2 * 4.4 / 9, -1.0 + 1 * 2.2 / 5        # h = 7, w = 2, d = 1 (just above the floor)
KS = (0, 1, -1, 2, -2, 3, -3)


DRIFT, DRIFT_DEG = 2e-5, math.degrees(1e-5)     # metres off the face at the camera, and the angle that brings the ray across it


def face_poses(axis, k):
    """A level camera 2e-5 m (+ k float32 steps) to one side of a voxel face, turned 1e-5 rad towards it: the centre column
    (h, w) or centre row (d) of the lattice crosses the face 2 m into the march, at 3e-6 grid units per step or less, and
    stays within the near-face margin (5.7e-6 grid units) for a few steps in the middle of a stretch."""
    if axis == "h":
        return (((0.25, float(steps_f32(FACE_Y - DRIFT, k)), -0.86), DRIFT_DEG, 0.0),)
    if axis == "w":
        return (((float(steps_f32(FACE_X + DRIFT, k)), 0.25, -0.86), 90.0 + DRIFT_DEG, 0.0),)
    return (((0.25, 2.7, float(steps_f32(FACE_Z - DRIFT, k))), 0.0, DRIFT_DEG),)


@pytest.mark.parametrize("mode", ("pixgrid", "explicit"))
@pytest.mark.parametrize("inv_s", (20.0, 200.0))
@pytest.mark.parametrize("S", (33, 64))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("axis", ("h", "w", "d"))
def test_near_face_inside_a_stretch(hip, axis, k, S, inv_s, mode):
    """the face-cold placements over the floor: near-face steps that fall inside a provable stretch"""
    rays = lattice(24, 16, 1, face_poses(axis, k))
    case = ("face", axis, k, mode, S, inv_s)
    kind = "floor" if inv_s == 20.0 else "floor200"
    n = wave_counts(scene_sdf(kind), mapping(), AABB, S, inv_s, rays, mode)
    _show(case, n)
    assert n["low_near_face"] > 0 and n["low_proven"] > 0, (case, n)
    got, ref = both_routes(volume(kind), rays, mode, AABB, S, inv_s)
    assert_equal(got, ref, case)


@pytest.mark.parametrize("face_safe", (True, False), ids=("face_safe", "no_face_safe"))
def test_slab(hip, face_safe):
    """the slab scene of tests/test_render_skip_run_gpu.py: provable steps inside the slab, free space on both sides"""
    rays, S, inv_s = _sr.slab_rays(), 128, _sr.SLAB_INV_S
    case = ("slab", face_safe)
    n = wave_counts(_sr.slab_sdf(), _sr.small_mapping(), _sr.AABB, S, inv_s, rays, "pixgrid", face_safe)
    _show(case, n)
    assert n["low_proven"] > 0 and n["skip"] > 0, (case, n)
    got, ref = both_routes(_sr.small_volume("slab", inv_s), rays, "pixgrid", _sr.AABB, S, inv_s, face_safe=face_safe)
    assert_equal(got, ref, case)
    assert float(got["acc"].max()) > 0.999
