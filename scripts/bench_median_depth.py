"""Time the median-depth launch (selfocc_render_median) against what there was before it, in ONE process.

Two frames, both 6 x 450 x 800 = 2.16 M pixel-grid rays x 256 samples, seeded synthetic scenes (selfocc_amd/synthetic.py):
  nuscenes_depth  the depth-evaluation frame: 257 x 257 x 31 SDF volume, no features (config/nuscenes/nuscenes_depth.py)
  nuscenes_occ    the occupancy head: 257 x 257 x 25 SDF volume + 24 float32 feature channels (config/nuscenes/nuscenes_occ.py)
Three variants, alternated inside every round:
  (a) median      render_median_depth: one launch, a ray stops at its crossing
  (b) per_sample  the route there was: render_rays(per_sample=True) in row-block chunks of ~90 000 rays (NeuSHead._normal_vis's
                  chunking), then torch.cumsum / searchsorted / gather on the (rays, S) weights
  (c) exact       render_rays(exact=True) of the SDF-only volume: a full canonical march of every ray, the yardstick
A figure is the median over the warm rounds of the device-event time of one call (min - max of the rounds beside it); the
garbage collector is off while rounds run.

Results: the rays on which (a) and (b) name another sample.  torch.cumsum on the GPU is a parallel scan: it adds the weights
in another order than the definition (sequential float32), so (b) is compared twice: as written (`disagree_cumsum`) and with
the running sum taken column by column in float32 (`disagree_sequential`, the definition itself, index and depth bit for bit; it
must be 0 and the script fails otherwise).  Both comparisons run chunk by chunk, on the very rays of (b).
`early_exit_share` = rays whose crossing comes before the last sample.

    python scripts/bench_median_depth.py [--rounds 5] [--out profiles/median_depth_bench.jsonl]
"""
import argparse
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
from selfocc_amd.render import RaySet, SDFVolume, render_median_depth, render_rays  # noqa: E402

CHUNK_RAYS = 90000
EVAL_LATTICE = (450, 800)          # rows, columns of the evaluation ray lattice of both configs
FRAMES = {                         # name -> (synthetic config, n_rgb, n_sem)
    'nuscenes_depth': ('cfg6', 0, 0),
    'nuscenes_occ': ('cfg5', 3, 21),
}


def chunks_of(rays):
    n = min(max(1, -(-rays.n_rays // CHUNK_RAYS)), rays.ny)
    return [sdist.shard_rays(rays, k, n) for k in range(n)], [sdist.row_block(rays.ny, k, n) for k in range(n)]


def frame_order(parts, rows, rays):
    """row-block chunks of every camera back to (camera, row, column) order"""
    n_cams = rays.img2lidar.shape[0]
    return torch.cat([p.reshape(n_cams, b - a, rays.nx) for p, (a, b) in zip(parts, rows)], 1).reshape(-1)


def crossing(w, ts, sequential):
    """(depth, index) of the first sample whose running weight sum reaches 0.5, from (rays, S) tensors on the GPU"""
    S = w.shape[1]
    if sequential:          # the definition: c_i = c_{i-1} + w_i, one float32 addition per sample
        c = torch.zeros(w.shape[0], device=w.device)
        j = torch.full((w.shape[0],), S - 1, dtype=torch.int64, device=w.device)
        found = torch.zeros(w.shape[0], dtype=torch.bool, device=w.device)
        for i in range(S):
            c = c + w[:, i]
            hit = (c >= 0.5) & ~found
            j = torch.where(hit, torch.full_like(j, i), j)
            found |= hit
    else:
        c = torch.cumsum(w, dim=-1)
        half = torch.full((w.shape[0], 1), 0.5, device=w.device)
        j = torch.searchsorted(c, half, side='left').squeeze(-1).clamp_(max=S - 1)
    return torch.gather(ts, 1, j[:, None]).squeeze(1), j.to(torch.int32)


def per_sample_route(vol, rays, cfg):
    subs, rows = chunks_of(rays)
    depth, index = [], []
    for sub in subs:
        o = render_rays(vol, sub, cfg, per_sample=True)
        dep, j = crossing(o['weights'], o['ts'], sequential=False)
        depth.append(dep); index.append(j)
    return frame_order(depth, rows, rays), frame_order(index, rows, rays)


def disagreements(vol, rays, cfg):
    """(a) against (b) on the SAME rays, chunk by chunk: a row block restates its pixel rows as iy * sy + (oy + r0 * sy), which
    rounds differently from the frame's (iy + r0) * sy + oy when sy is no power of two, so a chunk's rays are not bit for bit
    the frame's.  Returns (rays that differ from the sequential float32 definition in index or depth, rays whose index
    differs from the torch.cumsum route)."""
    n_seq = n_cumsum = 0
    for sub in chunks_of(rays)[0]:
        got = render_median_depth(vol, sub, cfg, want_index=True)
        o = render_rays(vol, sub, cfg, per_sample=True)
        dep, j = crossing(o['weights'], o['ts'], sequential=True)
        n_seq += int(((got['median_index'] != j) | (got['median_depth'].view(torch.int32) != dep.view(torch.int32))).sum())
        n_cumsum += int((got['median_index'] != crossing(o['weights'], o['ts'], sequential=False)[1]).sum())
    return n_seq, n_cumsum


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
    ap.add_argument("--frames", default=",".join(FRAMES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_depth_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_median_depth.py measures on the GPU"
    d = torch.device("cuda:0")
    lines = []
    for name in args.frames.split(","):
        scene, n_rgb, n_sem = FRAMES[name]
        vol = sy.make_volume(scene, n_rgb=n_rgb, n_sem=n_sem, seed=1).to(d)
        (ny, nx), (img_h, img_w) = EVAL_LATTICE, sy.CONFIGS[scene]['img']
        rays = RaySet(img2lidar=sy.make_cameras(scene).to(d), nx=nx, ny=ny, sx=img_w / nx, sy=img_h / ny)
        cfg = sy.make_render_config(scene)
        cfg_exact = sy.make_render_config(scene, exact=True)
        sdf_only = SDFVolume(vol.mapping, vol.sdf)
        assert rays.n_rays == 2160000 and cfg.n_samples == 256
        variants = {
            'median': lambda: render_median_depth(vol, rays, cfg, want_index=True),
            'per_sample': lambda: per_sample_route(vol, rays, cfg),
            'exact': lambda: render_rays(sdf_only, rays, cfg_exact),
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
        j = variants['median']()['median_index']
        n_seq, n_cumsum = disagreements(vol, rays, cfg)
        torch.cuda.synchronize()
        res = dict(frame=name, volume=list(vol.sdf.shape), feat_channels=0 if vol.feat is None else vol.feat.shape[-1],
                   n_rays=rays.n_rays, n_samples=cfg.n_samples, chunk_rays=CHUNK_RAYS, n_chunks=len(chunks_of(rays)[0]),
                   rounds=args.rounds, warmup=args.warmup, gpu=torch.cuda.get_device_name(0),
                   disagree_sequential=n_seq, disagree_cumsum=n_cumsum,
                   early_exit_share=round(float((j < cfg.n_samples - 1).float().mean()), 4),
                   mean_index=round(float(j.float().mean()), 2))
        for k, v in times.items():
            res[f'{k}_ms'] = round(statistics.median(v), 3)
            res[f'{k}_ms_min_max'] = [round(min(v), 3), round(max(v), 3)]
        res['median_over_exact'] = round(res['median_ms'] / res['exact_ms'], 3)
        res['per_sample_over_median'] = round(res['per_sample_ms'] / res['median_ms'], 1)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del vol, sdf_only
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")
    bad = [r['frame'] for r in lines if r['disagree_sequential'] != 0]
    assert not bad, f"the median launch and the sequential float32 definition disagree on {bad}"


if __name__ == "__main__":
    main()
