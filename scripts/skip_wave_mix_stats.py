"""CPU: which waves of the benchmark frame are resident together in the skip marcher's launch.
The march of so_march_fast_ahead restated in float32 numpy (tests/test_render_skip_low_mode_gpu.py: wave_tables, walk_wave),
as scripts/skip_low_mode_stats.py does.  Per wave of the cfg2 frame: full (interpolated) and free (skipped) steps, and a cost
in vector instructions, 67 * full + 16 * free + 400 (a proven low trip, a free step of the run loop, prelude and epilogue:
DESIGN 3.1, rounds 14 and 15).  Printed per camera by tile row (a row of 16-pixel blocks = two rows of 8 x 8 waves), then
the percentiles of the cost over all waves, then the share of the free steps in the step cost of consecutive windows of
the dispatch order (blocks x fastest) for three orders of the rows: camera by camera (grid (tiles_x, tiles_y, n_cams), the
order up to round 14), rows outermost (grid (tiles_x, n_cams, tiles_y), shipped in round 15: with one camera it is the
same order) and camera by camera with the rows taken alternately from the two ends of the image (measured 4 % slower).
    python scripts/skip_wave_mix_stats.py [--cams 0] [--inv-s 20,200] [--window 200]      (--cams 0,1,2,3,4,5: the frame)"""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from selfocc_amd import synthetic as sy
from selfocc_amd.render import RaySet

spec = importlib.util.spec_from_file_location("low_mode_tests", os.path.join(ROOT, "tests", "test_render_skip_low_mode_gpu.py"))
t = importlib.util.module_from_spec(spec)
spec.loader.exec_module(t)

ap = argparse.ArgumentParser()
ap.add_argument("--cams", default="0")
ap.add_argument("--inv-s", default="20,200")
ap.add_argument("--chunk", type=int, default=256, help="waves per pass")
ap.add_argument("--window", type=int, default=200, help="blocks per window of the dispatch order")
args = ap.parse_args()

V_FULL, V_FREE, V_FIXED = 67, 16, 400


def tile_row(r, tiles_y):
    """the alternating order of round 15 (not shipped): dispatch row -> tile row"""
    return tiles_y - 1 - r // 2 if r & 1 else r // 2


cfg = sy.CONFIGS["cfg2"]
vol = sy.make_volume("cfg2")
rays = sy.make_rays("cfg2")
S, aabb = cfg["n_samples"], cfg["aabb"]
sdf = vol.sdf.numpy()
abi_map = vol.mapping.to_abi()
wx, wy = (rays.nx + 7) // 8, (rays.ny + 7) // 8            # waves of a camera: wy rows of wx
tiles_x, tiles_y = (rays.nx + 15) // 16, (rays.ny + 15) // 16
cams = [int(v) for v in args.cams.split(",")]
for inv_s in (float(v) for v in args.inv_s.split(",")):
    codes, _ = t._sr.skip_codes_torch(vol.sdf, vol.mapping, aabb, S, inv_s)
    codes = codes.numpy()
    per_cam = {}
    entries = 0
    for cam in cams:
        one = RaySet(img2lidar=rays.img2lidar[cam:cam + 1], nx=rays.nx, ny=rays.ny, sx=rays.sx, sy=rays.sy)
        e = sy.explicit_rays(one)
        o, d = e.origins.numpy().astype(np.float32), e.dirs.numpy().astype(np.float32)
        lanes = t.wave_lanes(one, "pixgrid")                 # wave rows top to bottom, x fastest
        full, free = np.zeros(lanes.shape[0], np.int64), np.zeros(lanes.shape[0], np.int64)
        for at in range(0, lanes.shape[0], args.chunk):
            part = lanes[at:at + args.chunk]
            tab, i_lo, i_hi = t.wave_tables(sdf, codes, abi_map, aabb, S, inv_s, o, d, part)
            for w in range(part.shape[0]):
                c = t.walk_wave(S, int(i_lo[w]), int(i_hi[w]), tab, w)
                full[at + w], free[at + w] = c["full"], c["skip"]
                entries += c["low_entries"]
        per_cam[cam] = (full.reshape(wy, wx), free.reshape(wy, wx))
    print(f"cfg2, inv_s {inv_s:g}, cameras {args.cams}: {rays.nx} x {rays.ny} rays, {wx} x {wy} waves and "
          f"{tiles_x} x {tiles_y} blocks per camera; cost = {V_FULL} * full + {V_FREE} * free + {V_FIXED}")
    for cam, (full, free) in per_cam.items():
        print(f" camera {cam}: tile row, full steps / wave (min mean max), free steps / wave (min mean max), cost / wave (mean)")
        for r in range(tiles_y):
            fu, fr = full[2 * r:2 * r + 2].ravel(), free[2 * r:2 * r + 2].ravel()
            cost = V_FULL * fu + V_FREE * fr + V_FIXED
            print(f"  {r:3d}   {fu.min():4d} {fu.mean():6.1f} {fu.max():4d}   {fr.min():4d} {fr.mean():6.1f} {fr.max():4d}   {cost.mean():7.0f}")
    full = np.concatenate([per_cam[c][0].ravel() for c in cams])
    free = np.concatenate([per_cam[c][1].ravel() for c in cams])
    cost = V_FULL * full + V_FREE * free + V_FIXED
    n = full.size
    print(f" all {n} waves: full {full.mean():.1f}, free {free.mean():.1f}, low-mode entries {entries / n:.2f} per wave; "
          f"{100 * np.mean(full == 0):.1f} % of the waves interpolate no step")
    print(" cost percentiles: " + ", ".join(f"p{p} {np.percentile(cost, p):.0f}" for p in (5, 25, 50, 75, 95, 100)))
    # the dispatch order: blocks x fastest; a block = 2 x 2 waves
    rows, alt = list(range(tiles_y)), [tile_row(r, tiles_y) for r in range(tiles_y)]
    assert sorted(alt) == rows
    orders = (("camera by camera", [(c, r) for c in cams for r in rows]),
              ("rows outermost", [(c, r) for r in rows for c in cams]),
              ("alternating rows", [(c, r) for c in cams for r in alt]))
    for name, order in orders:
        fu, fr = [], []
        for cam, row in order:
            for bx in range(tiles_x):
                sl = (slice(2 * row, 2 * row + 2), slice(2 * bx, 2 * bx + 2))
                fu.append(per_cam[cam][0][sl].sum())
                fr.append(per_cam[cam][1][sl].sum())
        fu, fr = np.array(fu), np.array(fr)
        shares = []
        for at in range(0, fu.size, args.window):
            a, b = fu[at:at + args.window].sum(), fr[at:at + args.window].sum()
            shares.append(V_FREE * b / max(V_FULL * a + V_FREE * b, 1))
        print(f" {name:16s}: share of the free steps in the step cost per window of {args.window} blocks: "
              + " ".join(f"{s:.2f}" for s in shares))
