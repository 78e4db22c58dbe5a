"""Time NeuS hierarchical up-sampling (selfocc_render_upsample + the march on its edges) against uniform
sampling, in ONE process, SDF-only volumes (the sampler reads nothing else), seeded synthetic scenes (selfocc_amd/synthetic.py):

  nuscenes_occ_train   the nuscenes_occ training shape: 6 x 48 x 100 = 28 800 lattice rays, 257 x 257 x 25 volume
  nuscenes_depth_eval  the nuscenes_depth evaluation frame: 6 x 450 x 800 = 2.16 M lattice rays, 257 x 257 x 31 volume

Variants, alternated inside every round; a figure is the median over the warm rounds of the device-event time of one call:
  sampler        upsample_edges at 64 + 64 in 4 steps, row-block chunks whose edge buffer stays below 256 MB (NeuSHead.render's)
  upsampled      sampler + render_rays(edges=) of every chunk: what a frame at 64 + 64 costs
  exact128       the canonical (exact=True) render at 128 uniform samples: the yardstick of the sampler (the same number of SDF
                 lookups, no scans)
  exact64        the canonical render at 64 uniform samples: what the march on the sampler's edges would cost without the sampler
  uniform256     the shipped 256 uniform samples on the default (fast) route

    python scripts/bench_upsample.py [--rounds 5] [--out profiles/upsample_bench.json]
"""
import argparse
import dataclasses
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from selfocc_amd import dist as sdist, synthetic as sy  # noqa: E402
from selfocc_amd.render import RaySet, SDFVolume, render_rays, upsample_edges  # noqa: E402

S0, M, K, BASE_VARIANCE = 64, 64, 4, 64.0
EDGE_BYTES = 256 << 20
SHAPES = {                         # name -> (synthetic config, (rows, columns) of the ray lattice)
    'nuscenes_occ_train': ('cfg5', (48, 100)),
    'nuscenes_depth_eval': ('cfg6', (450, 800)),
}


def chunks_of(rays):
    n = -(-(rays.n_rays * (S0 + M + 1) * 4) // EDGE_BYTES)
    n = min(max(1, n), rays.ny)
    return [sdist.shard_rays(rays, k, n) for k in range(n)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_upsample.py measures on the GPU"
    d = torch.device("cuda:0")
    results = []
    for name in args.shapes.split(","):
        scene, (ny, nx) = SHAPES[name]
        vol = sy.make_volume(scene, seed=1).to(d)
        vol = SDFVolume(vol.mapping, vol.sdf)
        img_h, img_w = sy.CONFIGS[scene]['img']
        rays = RaySet(img2lidar=sy.make_cameras(scene).to(d), nx=nx, ny=ny, sx=img_w / nx, sy=img_h / ny)
        cfg = sy.make_render_config(scene)
        cfg64 = dataclasses.replace(cfg, n_samples=S0)
        cfg128x, cfg64x = dataclasses.replace(cfg, n_samples=S0 + M, exact=True), dataclasses.replace(cfg, n_samples=S0, exact=True)
        subs = chunks_of(rays)
        sampler = lambda: [upsample_edges(vol, sub, cfg64, M, K, BASE_VARIANCE) for sub in subs][-1]
        upsampled = lambda: [render_rays(vol, sub, cfg64, edges=upsample_edges(vol, sub, cfg64, M, K, BASE_VARIANCE)) for sub in subs][-1]
        variants = {
            'sampler': sampler,
            'upsampled': upsampled,
            'exact128': lambda: render_rays(vol, rays, cfg128x),
            'exact64': lambda: render_rays(vol, rays, cfg64x),
            'uniform256': lambda: render_rays(vol, rays, cfg),
        }
        times = {k: [] for k in variants}
        gc.collect()
        gc.disable()
        try:
            for rnd in range(args.warmup + args.rounds):
                for k, fn in variants.items():
                    ms, _ = timed(fn)
                    if rnd >= args.warmup:
                        times[k].append(ms)
        finally:
            gc.enable()
        edges = upsample_edges(vol, subs[0], cfg64, M, K, BASE_VARIANCE)
        widths = edges[:, 1:] - edges[:, :-1]
        res = dict(shape=name, volume=list(vol.sdf.shape), n_rays=rays.n_rays, samples=[S0, M, K], base_variance=BASE_VARIANCE,
                   n_chunks=len(subs), rounds=args.rounds, warmup=args.warmup, gpu=torch.cuda.get_device_name(0),
                   # how far the samples moved: the share of bins narrower than half a uniform bin of 128
                   narrow_bin_share=round(float((widths < 0.5 / (S0 + M)).float().mean()), 4))
        for k, v in times.items():
            res[f'{k}_ms'] = round(statistics.median(v), 3)
            res[f'{k}_ms_min_max'] = [round(min(v), 3), round(max(v), 3)]
        res['sampler_over_exact128'] = round(res['sampler_ms'] / res['exact128_ms'], 3)
        res['upsampled_over_uniform256'] = round(res['upsampled_ms'] / res['uniform256_ms'], 3)
        print(json.dumps(res), flush=True)
        results.append(res)
        del vol
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
