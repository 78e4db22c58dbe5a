"""GPU: the exit of the code-ahead skip marcher (csrc/render_fwd.hip, so_march_fast_ahead, kSpentPre).

The marcher leaves a wave once no later step can change a bit of acc, dsum, best_w or best_t in any lane ("every lane is
spent"): T * 2^25 < acc, fl((T * 2^26) * tb) < |dsum| and T <= best_w, looked at only once every lane has T < 2^-24.  The
reference is ``ahead=False`` (so_march_fast), which marches until every lane has T < 1e-10: if the new rule left a wave one
step too early, some output would differ in a bit.  All five outputs must be torch.equal, with the output buffers
pre-filled with NaN, on both launch kinds, with and without face-safe cell selection, at inv_s 20 and 200, inv_s passed by
value and read from the device.

The scenes live in a 24 x 24 x 8 volume with 0.4 m cells in x and y under a 24 x 16 lattice (6 tiles of 8 x 8 rays):

  * floor-D, D in {0.6, 0.9, 1.2, 2.0}: a floor at z = 0 and D metres of solid under it, seen from 0.8 m above.  Inside the
    solid T ~ sigmoid(inv_s * (sdf - dt / 2)), so at inv_s 20 neither rule fires above the 0.6 m floor, and under the deeper ones
    the new rule fires one to three steps before the old one (at S = 9 over the 1.2 m floor the new one alone); at S = 9, 17,
    33, 64 and 128 the exit moves through the sure loop and both halves of low mode;
  * near: the camera one step above the floor, so dsum is ~1e-2 of tb and condition (b) holds 6 - 7 e-foldings of T after
    (a).  ((b) is the last to hold in every scene: dsum <= ~acc * tb makes it imply (a).  A build without (b) fails here, in
    the oblique scene and under the 1.2 m floor at S = 128; a build with (a) at 2^-23 or without (c) cannot fail anywhere,
    since (b) implies that looser (a) and best_w >= acc / S makes (a) imply (c).)
  * hole: a shaft of free space through the solid: the lanes that look down it never meet a surface and their tile must
    march to the end (their acc keeps registering the free-space weights);
  * oblique: a camera that looks along the floor, so that the lanes of a tile are spent over a spread of >= 8 steps;
  * nan: a NaN corner in the solid on some lanes' paths (so_alpha_fast turns it into alpha ~ 1);
  * above: the launch's box reaches 1.6 m above the grid, so the waves have no sure range and march, and leave, in the
    general loop;
  * slab: a slab with free space under it, its thickness tuned (on the CPU restatement below) so that the tile's last lane
    is spent in the middle of the free-space run behind it: the exit inside the run loop.

No case is vacuous.  `spent_tables` is the float32 numpy restatement of the march of tests/test_render_skip_low_mode_gpu.py
(wave_tables) carried on with T, acc, dsum and best_w, and `walk_exit` walks a wave through the loops as walk_wave does and
says after which step, and in which loop, a rule lets it go.  Only these counts are used, never the restatement's values.
"""
import collections
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from selfocc_amd import synthetic as sy
from selfocc_amd._lib import check, current_stream, lib, ptr
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import RenderConfig, SDFVolume, _brick_workspace, marshal_render_args

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_low_mode_scenes", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  "test_render_skip_low_mode_gpu.py"))
_lm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_lm)
_sr = _lm._sr

KEYS = _lm.KEYS
f32, f64 = np.float32, np.float64
fma32 = _lm.fma32
TOP = 1.0                      # the grid's top; the floor is at z = 0
NX, NY = 24, 16
K_SPENT_PRE = f32(2.0 ** -24)
PLACES = ("general", "sure", "run", "low_a", "low_b")
DOWN = (((4.6, 4.6, 0.8), 30.0, -90.0),)
# Half the slab's thickness.  Behind the slab T falls by 1e-5 a step, so the last lane is spent inside the free-space run only
# if it comes out of the slab within ~5e-4 of its threshold: found by bisection on the restatement (exit after steps 102 -
# 105 of a run that spans steps 90 - 127; one float32 step of the value moves the exit by a step or two).
SLAB_HALF = 0.0768682


def spent_mapping(depth):
    return GridMeterMapping(nonlinear_mode='linear', h_size=[23, 0], h_range=[9.2, 0], h_half=True, w_size=[23, 0],
                            w_range=[9.2, 0], w_half=True, d_size=[7, 0], d_range=[-depth, TOP, TOP])


def aabb_of(depth, top=TOP):
    return (0.0, 0.0, -depth, 9.2, 9.2, top)


def _noise(seed):
    return torch.randn((24, 24, 8), generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def scene_sdf(kind, depth):
    xyz = sy.grid_points_meter(spent_mapping(depth))
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    sdf = z + 0.004 * _noise(5)
    if kind == "hole":          # a shaft of free space, 1.2 m wide, under the left of the image
        shaft = ((x - 4.6).abs() < 0.7) & ((y - 3.8).abs() < 0.7)
        sdf = torch.where(shaft, torch.full_like(sdf, 3.0), sdf)
    elif kind == "nan":
        sdf = sdf.clone()
        sdf[12, 11, 2] = float("nan")       # in the solid, under the middle of the image
        sdf[10, 13, 6] = float("nan")       # and in the free space above it
    elif kind == "slab":        # free space above and below
        sdf = (z - xyz[0, 0, 3, 2]).abs() - SLAB_HALF + 0.0 * x
    elif kind != "floor":
        raise KeyError(kind)
    return sdf.contiguous().float()


# (label, scene, depth, box top, poses, S): the launches of this file
def _cases():
    out = []
    for depth in (0.6, 0.9, 1.2, 2.0):
        for S in (64, 9, 17, 33, 128):
            out.append((f"floor{depth}_S{S}", "floor", depth, TOP, DOWN, S))
    out.append(("near", "floor", 2.0, TOP, (((4.6, 4.6, 0.03), 30.0, -90.0),), 64))
    out.append(("hole", "hole", 2.0, TOP, DOWN, 64))
    out.append(("oblique", "floor", 2.0, TOP, (((0.4, 0.6, 0.5), 45.0, -24.0),), 128))
    out.append(("nan", "nan", 2.0, TOP, DOWN, 64))
    out.append(("above", "floor", 2.0, TOP + 1.6, (((4.6, 4.6, 2.4), 30.0, -90.0),), 64))
    out.append(("slab", "slab", 2.0, TOP, DOWN, 128))
    return out


CASES = _cases()


def rays_of(poses):
    return _lm.lattice(NX, NY, len(poses), poses)


# ---- the launch -------------------------------------------------------------------------------------------------------
def launch(vol, rays, cfg):
    """render_fwd with the brick workspace whatever the size of the batch, into buffers that hold NaN"""
    a, out, _keep = marshal_render_args(vol, rays, cfg)
    for k in KEYS:
        out[k].fill_(float("nan"))
    a.sdf_brick = ptr(_brick_workspace(vol.sdf))
    check(lib().selfocc_render_fwd(a, current_stream(vol.sdf.device)), "selfocc_render_fwd")
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in KEYS}


def both_routes(dvol, r, aabb, S, inv_s, how, face_safe):
    d = dvol.sdf.device
    ref = launch(dvol, r, RenderConfig(aabb=aabb, n_samples=S, inv_s=inv_s, ahead=False, face_safe=face_safe))
    if how == "device":     # the kernels must read the device's value: the host field holds another one
        cfg = RenderConfig(aabb=aabb, n_samples=S, inv_s=0.5 * inv_s, face_safe=face_safe,
                           inv_s_dev=torch.tensor([inv_s], dtype=torch.float32, device=d))
    else:
        cfg = RenderConfig(aabb=aabb, n_samples=S, inv_s=inv_s, face_safe=face_safe)
    return launch(dvol, r, cfg), ref


def assert_equal(got, ref, case):
    """bit for bit, NaN included (the nan scene may store some)"""
    bad = {k: int((got[k].view(torch.int32) != ref[k].view(torch.int32)).sum()) for k in KEYS}
    print(f"[spent-exit] {case}: rays {ref['acc'].numel()}; differing values {bad}")
    for k in KEYS:
        assert torch.equal(got[k].view(torch.int32), ref[k].view(torch.int32)), (case, k, bad[k])


# ---- the march, restated on the CPU -------------------------------------------------------------------------------
def spent_tables(sdf, codes, mapping_abi, aabb, S, inv_s, o, d, lanes):
    """wave_tables of the low-mode test, with the lane state the exit rules look at.  Returns the same dict of (n_waves, S)
    bool arrays with `exit` (after the step: every lane T < 1e-10) and `exit_new` (every lane T < 2^-24, and every lane spent
    or `exit`), `first_spent` (n_waves, 64: the first step after which the lane is spent, S if never; -1 for a lane without
    a ray), `b_last` / `c_last` (n_waves, 64: at some step condition (b) / (c) alone kept the lane from being spent), and the
    sure range (i_lo, i_hi) of every wave."""
    H, W, D = sdf.shape
    valid = lanes >= 0
    li = np.where(valid, lanes, 0)
    o, d = o[li], d[li]
    lo, hi = np.array(aabb[:3], f32), np.array(aabb[3:], f32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        inv = f32(1.0) / (d + f32(1e-6))
        ta, tb_ = (lo - o) * inv, (hi - o) * inv
        tnear = np.maximum(np.minimum(ta, tb_).max(-1), f32(0.0))
        tfar = np.maximum(np.maximum(ta, tb_).min(-1), tnear + f32(1e-6))
        dt = (tfar - tnear) / f32(S)
        hdt = f32(0.5) * dt
        maxdim = max(H, W, D)
        face_m = f32(3.0) * f32(1.1920929e-7) * f32(1 << maxdim.bit_length())
        fi = np.arange(S, dtype=f32)
        step = fi[None, None, :] * dt[..., None]
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
        v = [sdf[h0 + a, w0 + b, d0 + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)]
        s2 = f32(inv_s) * _lm.LOG2E
        thr = _lm.LOW_C * (f32(1.0) / s2)
        provable = ((v[0] <= thr) & vmask).any(1)
        near = ((np.maximum(np.maximum(np.abs(fr[0] - f32(0.5)), np.abs(fr[1] - f32(0.5))), np.abs(fr[2] - f32(0.5))) > f32(0.5) - face_m) & vmask).any(1)
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
        hs = np.fmin(cosv, f32(0.0)) * (hdt * s2)[..., None]              # fminf: a NaN operand is dropped
        ea, eb = np.exp2(np.fmin(hs - xs, f32(60.0))), np.exp2(np.fmin(-hs - xs, f32(60.0)))
        p = f32(1.0) + ea
        alpha = np.fmin(fma32(eb - ea, f32(1.0) / (f32(1.0) + eb), f32(1e-5) * p) / fma32(np.full_like(p, f32(1e-5)), p, np.ones_like(p)), f32(1.0))
        hint = (~lane_free | ~vmask).all(1)
        t_first = tnear + hdt
        t_bound = np.maximum(np.abs(t_first), np.abs(fma32(np.full_like(dt, f32(S - 1)), dt, t_first)))
        T = np.ones(lanes.shape, f32)
        acc, dsum, best_w = np.zeros(lanes.shape, f32), np.zeros(lanes.shape, f32), np.full(lanes.shape, f32(-1.0))
        exit_, exit_new = np.zeros(free.shape, bool), np.zeros(free.shape, bool)
        first_spent = np.where(valid, S, -1)
        b_last, c_last = np.zeros(lanes.shape, bool), np.zeros(lanes.shape, bool)
        for i in range(S):
            a_i = np.where(free[:, None, i], _lm.K_ALPHA_FREE, alpha[..., i]).astype(f32)
            w = a_i * T
            T = T * ((f32(1.0) - a_i) + f32(1e-7))
            acc = acc + w
            dsum = fma32(w, fma32(np.full_like(dt, f32(i)), dt, t_first), dsum)
            best_w = np.where(w > best_w, w, best_w)
            ca, cb, cc = T * f32(2.0 ** 25) < acc, (T * f32(2.0 ** 26)) * t_bound < np.abs(dsum), T <= best_w
            spent = ca & cb & cc
            b_last |= ca & cc & ~cb & valid
            c_last |= ca & cb & ~cc & valid
            first_spent = np.where(spent & (first_spent == S), i, first_spent)
            exit_[:, i] = ((T < f32(1e-10)) | ~valid).all(1)
            exit_new[:, i] = ((T < K_SPENT_PRE) | ~valid).all(1) & ((spent | ~valid).all(1) | exit_[:, i])
    tab = dict(interior=interior, free=free, provable=provable, hint=hint, near=near, exit=exit_, exit_new=exit_new,
               first_spent=first_spent, b_last=b_last, c_last=c_last)
    n = min(_lm.K_SURE_SCAN, S)
    i_lo, i_hi = np.full(lanes.shape[0], S), np.full(lanes.shape[0], -1)
    for wv in range(lanes.shape[0]):
        first = np.flatnonzero(interior[wv, :n])
        if first.size:
            last = [k for k in range(S - 1, max(S - n, first[0]) - 1, -1) if interior[wv, k]]
            if last:
                i_lo[wv], i_hi[wv] = first[0], last[0]
    return tab, i_lo, i_hi


def walk_exit(S, i_lo, i_hi, t, w, exit_, face_safe=True):
    """One wave through the loops of so_march_fast_ahead (walk_wave of the low-mode test, which counts the step kinds) under
    the exit rule `exit_` (a row of t["exit"] or t["exit_new"]).  Returns (place, i): the loop whose test lets the wave go and
    the last step it composited, or (None, S - 1) for a wave that marches to the end."""
    free, prov, hint, near = t["free"][w], t["provable"][w], t["hint"][w], t["near"][w]
    hinted = 0
    i = 0
    while i < min(i_lo, S):                                   # head (or the whole march of a wave without a sure range)
        i += 1
        if i >= S:
            return None, S - 1
        if exit_[i - 1]:
            return "general", i - 1
    while i < i_hi:                                           # sure loop: the two halves of its body, then low mode's entry
        entered = False
        for half in (0, 1):
            sk = bool(free[i])
            hinted = hinted + 1 if (not sk and hint[i]) else 0
            i += 1
            if exit_[i - 1]:
                return "sure", i - 1
            while sk and i < i_hi and free[i]:                # run loop
                i += 1
                if exit_[i - 1]:
                    return "run", i - 1
            if i >= i_hi:
                break
            entered = half == 1 and hinted >= _lm.ENTER_AFTER
        if entered:
            trip = 0
            while i + 1 < i_hi and not (face_safe and near[i]):
                proven = bool(prov[i])
                i += 1
                if exit_[i - 1]:
                    return ("low_a", "low_b")[trip & 1], i - 1
                trip += 1
                if not proven:
                    break
    while i < S:                                              # tail
        i += 1
        if i < S and exit_[i - 1]:
            return "general", i - 1
    return None, S - 1


@functools.lru_cache(maxsize=None)
def census(label, mode, inv_s, face_safe=True):
    """per wave of a case's launch: (place, last step) under the new rule, the same under the old one, the spread of the
    steps at which the wave's lanes are spent (None if some lane never is), and the number of lanes that condition (b) / (c)
    alone kept from being spent at some step"""
    _, kind, depth, top, poses, S = next(c for c in CASES if c[0] == label)
    sdf_t, mp, aabb, rays = scene_sdf(kind, depth), spent_mapping(depth), aabb_of(depth, top), rays_of(poses)
    codes, _ = _sr.skip_codes_torch(torch.nan_to_num(sdf_t, nan=-1.0), mp, aabb, S, inv_s)     # a NaN corner: code 0
    e = sy.explicit_rays(rays)
    lanes = _lm.wave_lanes(rays, mode)
    t, i_lo, i_hi = spent_tables(sdf_t.numpy(), codes.numpy(), mp.to_abi(), aabb, S, inv_s, e.origins.numpy().astype(f32),
                                 e.dirs.numpy().astype(f32), lanes)
    out = []
    for w in range(lanes.shape[0]):
        new = walk_exit(S, int(i_lo[w]), int(i_hi[w]), t, w, t["exit_new"][w], face_safe)
        old = walk_exit(S, int(i_lo[w]), int(i_hi[w]), t, w, t["exit"][w], face_safe)
        fs = t["first_spent"][w][lanes[w] >= 0]
        out.append((new, old, None if (fs == S).any() else int(fs.max() - fs.min()), int(t["b_last"][w].sum()), int(t["c_last"][w].sum())))
    return out


def totals(labels=None, modes=("pixgrid", "explicit"), inv_ss=(20.0, 200.0)):
    n = collections.Counter()
    for label, *_ in CASES:
        if labels is not None and label not in labels:
            continue
        for mode in modes:
            for inv_s in inv_ss:
                for (new, old, spread, nb, nc) in census(label, mode, inv_s):
                    n["waves"] += 1
                    n["b_last_lanes"] += nb
                    n["c_last_lanes"] += nc
                    if new[0] is not None:
                        n["early"] += 1
                        n[new[0]] += 1
                        n["earlier"] += new[1] < old[1]
                        n["steps_saved"] += old[1] - new[1]
                        assert new[1] <= old[1]
                        if spread is not None and spread >= 8:
                            n["spread_8"] += 1
                    assert old[0] is None or new[0] is not None
    return n


# ---- the cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("face_safe", (True, False), ids=("face_safe", "no_face_safe"))
@pytest.mark.parametrize("mode", ("pixgrid", "explicit"))
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_spent_exit_equals_old_rule(hip, case, mode, face_safe):
    label, kind, depth, top, poses, S = case
    d = torch.device("cuda:0")
    rays = rays_of(poses)
    r = _lm.on_gpu(sy.explicit_rays(rays) if mode == "explicit" else rays)
    dvol = SDFVolume(spent_mapping(depth), scene_sdf(kind, depth)).to(d)
    for inv_s in (20.0, 200.0):
        for how in ("value", "device"):
            got, ref = both_routes(dvol, r, aabb_of(depth, top), S, inv_s, how, face_safe)
            assert_equal(got, ref, (label, mode, face_safe, inv_s, how))
            assert not torch.isnan(got["nears"]).any() and not torch.isnan(got["fars"]).any()      # every ray was written
            if kind != "nan":
                assert torch.isfinite(got["depth"]).all() and torch.isfinite(got["acc"]).all()


def test_not_vacuous(hip):
    """The restatement's counts over the launches above: the new rule fires strictly earlier than the old one in at least a
    quarter of the waves that leave early, every loop's exit is taken, and each scene does what it is there for."""
    n = totals()
    print("[spent-exit] " + ", ".join(f"{k}={n[k]}" for k in ("waves", "early", "earlier", "steps_saved", "spread_8",
                                                               "b_last_lanes", "c_last_lanes") + PLACES))
    assert n["early"] > 0 and 4 * n["earlier"] >= n["early"], n
    for place in PLACES:
        assert n[place] > 0, (place, n)
    by = {label: census(label, "pixgrid", 20.0) for label in ("floor0.6_S64", "floor1.2_S9", "floor2.0_S64", "near", "hole",
                                                                "oblique", "nan", "above")}
    fired = lambda rule: rule[0] is not None
    assert not any(fired(c[0]) for c in by["floor0.6_S64"])                          # the box ends first
    assert any(fired(c[0]) and not fired(c[1]) for c in by["floor1.2_S9"])           # the new rule alone
    assert all(fired(c[0]) and fired(c[1]) and c[0][1] < c[1][1] for c in by["floor2.0_S64"])
    assert any(not fired(c[0]) for c in by["hole"]) and any(fired(c[0]) for c in by["hole"])
    assert any(fired(c[0]) and c[2] is not None and c[2] >= 8 for c in census("oblique", "explicit", 20.0))
    assert all(fired(c[0]) for c in by["nan"])
    assert all(fired(c[0]) and c[3] > 0 for c in by["near"])                         # lanes that (b) alone holds back
    assert all(c[0][0] == "general" for c in by["above"])
    assert all(c[0][0] == "run" and 95 <= c[0][1] <= 115 for c in census("slab", "pixgrid", 200.0))
