"""CPU: what the benchmark frame puts in front of a skip marcher that proves full steps from their corners.
The march of so_march_fast_ahead restated in float32 numpy (tests/test_render_skip_low_mode_gpu.py: wave_tables, walk_wave):
skip codes as sdf_brickify_kernel computes them, 8 x 8 pixel tiles, the wave-wide decisions and exit test.  Printed per wave
of the cfg2 frame, at inv_s 20 and 200: full and skip steps, the full steps the shipped predicate proves unskippable (some
lane's corner v0 <= C / s2, the test's LOW_C) and the share the 8-corner minimum and a two-corner form would prove, stretch
starts, and what a mode that leaves the code load out of proven steps does: entries, steps proven / unproven and kept /
unproven and skipped, near-face and range-end exits, vector-memory instructions per wave with and without it.
    python scripts/skip_low_mode_stats.py [--cams 0,3] [--inv-s 20,200]"""
import argparse
import collections
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from selfocc_amd import synthetic as sy
from selfocc_amd.render import RaySet

spec = importlib.util.spec_from_file_location("low_mode_tests", os.path.join(ROOT, "tests", "test_render_skip_low_mode_gpu.py"))
t = importlib.util.module_from_spec(spec)
spec.loader.exec_module(t)

ap = argparse.ArgumentParser()
ap.add_argument("--cams", default="0,3")
ap.add_argument("--inv-s", default="20,200")
ap.add_argument("--chunk", type=int, default=256, help="waves per pass")
args = ap.parse_args()

cfg = sy.CONFIGS["cfg2"]
vol = sy.make_volume("cfg2")
rays = sy.make_rays("cfg2")
S, aabb = cfg["n_samples"], cfg["aabb"]
sdf = vol.sdf.numpy()
abi_map = vol.mapping.to_abi()
for inv_s in (float(v) for v in args.inv_s.split(",")):
    codes, _ = t._sr.skip_codes_torch(vol.sdf, vol.mapping, aabb, S, inv_s)
    codes = codes.numpy()
    total = collections.Counter()
    few = collections.Counter()          # full wave-steps a cheaper predicate proves
    for cam in (int(v) for v in args.cams.split(",")):
        one = RaySet(img2lidar=rays.img2lidar[cam:cam + 1], nx=rays.nx, ny=rays.ny, sx=rays.sx, sy=rays.sy)
        e = sy.explicit_rays(one)
        o, d = e.origins.numpy().astype(np.float32), e.dirs.numpy().astype(np.float32)
        lanes = t.wave_lanes(one, "pixgrid")
        for at in range(0, lanes.shape[0], args.chunk):
            part = lanes[at:at + args.chunk]
            tab, i_lo, i_hi = t.wave_tables(sdf, codes, abi_map, aabb, S, inv_s, o, d, part, corner_forms=True)
            total["waves"] += part.shape[0]
            for w in range(part.shape[0]):
                total.update(t.walk_wave(S, int(i_lo[w]), int(i_hi[w]), tab, w))
            full = ~tab["free"] & tab["marched"]
            few["full"] += int(full.sum())
            for k in ("provable", "provable_8", "provable_2", "sdf_low", "hint"):
                few[k] += int((full & tab[k]).sum())
    n = total["waves"]
    print(f"cfg2, cameras {args.cams}, inv_s {inv_s:g}: {n} waves; per wave:")
    for k in ("full", "skip", "full_provable", "stretch_starts", "low_entries", "low_proven", "low_unproven_kept",
              "low_unproven_skipped", "low_near_face", "low_range_end", "vmem_parent", "vmem_low"):
        print(f"  {k:22s} {total[k] / n:8.2f}")
    print(f"  of the full wave-steps: corner v0 (shipped) proves {100 * few['provable'] / few['full']:.1f} %, the 8-corner minimum "
          f"{100 * few['provable_8'] / few['full']:.1f} %, min(v0, v7) {100 * few['provable_2'] / few['full']:.1f} %; some lane's "
          f"interpolated sdf * s2 <= C: {100 * few['sdf_low'] / few['full']:.1f} %; no lane free (the entry hint): "
          f"{100 * few['hint'] / few['full']:.1f} %")
    print(f"  vector-memory instructions: {100 * (total['vmem_low'] / total['vmem_parent'] - 1):+.1f} % with the mode")
