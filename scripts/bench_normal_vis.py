"""Time the rendered-normal launch (selfocc_render_normal) against the route there was, in ONE process.

The frame is the `nuscenes_depth` evaluation frame: 6 x 450 x 800 = 2.16 M pixel-grid rays x 256 samples on a 257 x 257 x 31 SDF
volume without features (config/nuscenes/nuscenes_depth.py), a seeded synthetic scene (selfocc_amd/synthetic.py).
Three variants, alternated inside every round:
  (a) normal      render_normal_vis: one launch, every ray marches its 256 samples canonically
  (b) per_sample  NeuSHead._normal_vis, the route there was and still is: render_rays(per_sample=True, want_grad_samples=True) in
                  row-block chunks of ~90 000 rays, then four torch ops on the (rays, S) weights and (rays, S, 3) gradients
  (c) depth       render_rays of the SDF-only volume: the depth render of the same frame (the skip marcher), for scale
A figure is the median over the warm rounds of the device-event time of one call (min - max of the rounds beside it); the
garbage collector is off while rounds run.

Results: `max_abs_diff` between (a) and (b) on the frame ((b) sums with torch.sum, in another order than the definition), and
`disagree_sequential`, the rays on which (a) differs in any bit from the definition (normal_vis_reference, on the host) applied
to the per-sample outputs of the first row-block chunk; it must be 0 and the script fails otherwise.

    python scripts/bench_normal_vis.py [--rounds 5] [--out profiles/normal_vis_bench.jsonl]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from selfocc_amd import dist as sdist, synthetic as sy  # noqa: E402
from selfocc_amd.model.head.neus_head import NeuSHead  # noqa: E402
from selfocc_amd.render import RaySet, SDFVolume, normal_vis_reference, render_normal_vis, render_rays  # noqa: E402

CHUNK_RAYS = 90000
EVAL_LATTICE = (450, 800)          # rows, columns of the evaluation ray lattice
SCENE = 'cfg6'
PLAIN_HEAD = types.SimpleNamespace(up_steps=0)       # all NeuSHead._normal_vis reads of its head: no up-sampling


def disagreements(vol, rays, cfg):
    n = min(max(1, -(-rays.n_rays // CHUNK_RAYS)), rays.ny)
    sub = sdist.shard_rays(rays, 0, n)
    got = render_normal_vis(vol, sub, cfg)
    o = render_rays(vol, sub, cfg, per_sample=True, want_grad_samples=True)
    want = normal_vis_reference(o['weights'].cpu(), o['grad'].cpu())
    return int((got.cpu().view(torch.int32) != want.view(torch.int32)).any(1).sum()), sub.n_rays


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_vis_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_normal_vis.py measures on the GPU"
    d = torch.device("cuda:0")
    vol = sy.make_volume(SCENE, seed=1).to(d)
    (ny, nx), (img_h, img_w) = EVAL_LATTICE, sy.CONFIGS[SCENE]['img']
    rays = RaySet(img2lidar=sy.make_cameras(SCENE).to(d), nx=nx, ny=ny, sx=img_w / nx, sy=img_h / ny)
    cfg = sy.make_render_config(SCENE)
    sdf_only = SDFVolume(vol.mapping, vol.sdf)
    assert rays.n_rays == 2160000 and cfg.n_samples == 256 and vol.feat is None
    variants = {
        'normal': lambda: render_normal_vis(sdf_only, rays, cfg),
        'per_sample': lambda: NeuSHead._normal_vis(PLAIN_HEAD, sdf_only, rays, cfg, chunk_rays=CHUNK_RAYS),
        'depth': lambda: render_rays(sdf_only, rays, cfg),
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
    a, b = variants['normal'](), variants['per_sample']()
    acc = variants['depth']()['acc']
    n_seq, n_checked = disagreements(sdf_only, rays, cfg)
    torch.cuda.synchronize()
    res = dict(frame='nuscenes_depth', volume=list(vol.sdf.shape), n_rays=rays.n_rays, n_samples=cfg.n_samples,
               chunk_rays=CHUNK_RAYS, n_chunks=min(max(1, -(-rays.n_rays // CHUNK_RAYS)), rays.ny),
               rounds=args.rounds, warmup=args.warmup, gpu=torch.cuda.get_device_name(0),
               disagree_sequential=n_seq, rays_checked=n_checked, max_abs_diff=float((a - b).abs().max()),
               hit_share=round(float((acc > 0.5).float().mean()), 4))
    for k, v in times.items():
        res[f'{k}_ms'] = round(statistics.median(v), 3)
        res[f'{k}_ms_min_max'] = [round(min(v), 3), round(max(v), 3)]
    res['per_sample_over_normal'] = round(res['per_sample_ms'] / res['normal_ms'], 2)
    res['normal_over_depth'] = round(res['normal_ms'] / res['depth_ms'], 2)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    assert n_seq == 0, f"the normal launch and the sequential float32 definition disagree on {n_seq} of {n_checked} rays"


if __name__ == "__main__":
    main()
