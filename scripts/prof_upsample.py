"""Profiling target: the up-sampling launch (selfocc_render_upsample) alone, at 64 + 64 samples in 4 steps, on one
row-block chunk of the nuscenes_depth evaluation frame, beside the canonical 128-sample march of the same rays (its yardstick).

    rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES ... -- python scripts/prof_upsample.py [launches]
"""
import dataclasses
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from selfocc_amd import dist as sdist, synthetic as sy  # noqa: E402
from selfocc_amd.render import RaySet, SDFVolume, render_rays, upsample_edges  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    d = torch.device("cuda:0")
    vol = sy.make_volume("cfg6", seed=1).to(d)
    vol = SDFVolume(vol.mapping, vol.sdf)
    img_h, img_w = sy.CONFIGS["cfg6"]['img']
    rays = RaySet(img2lidar=sy.make_cameras("cfg6").to(d), nx=800, ny=450, sx=img_w / 800, sy=img_h / 450)
    sub = sdist.shard_rays(rays, 0, 5)                       # 432 000 rays: one chunk of NeuSHead.render
    cfg = dataclasses.replace(sy.make_render_config("cfg6"), n_samples=64)
    cfg128 = dataclasses.replace(cfg, n_samples=128, exact=True)
    for _ in range(n):
        upsample_edges(vol, sub, cfg, 64, 4, 64.0)
        render_rays(vol, sub, cfg128)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
