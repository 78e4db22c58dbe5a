"""Time the masked render kernels (any class count) against the shipped widths, in ONE process.

On the 257 x 257 x 25 volume of the shipped occupancy configs:
  eval      render_rays, default flags, 6 x 450 x 800 = 2.16 M rays x 256 samples (pixel grid: brick re-pack + LDS-staged kernel)
  train_fwd render_rays(per_sample=True), the 6 x 48 x 100 = 28 800-ray training lattice x 256 samples
  bwd       selfocc_render_bwd through render_rays_autograd's backward, binned scatter, same lattice
at n_sem = 5 and 21 (the shipped kernels: the yardstick) and n_sem = 4, 11, 20 (masked: 8-, 16- and 24-float rows).  The
variants alternate inside every round; a figure is the median over the warm rounds of the mean device-event time per call,
with the min - max of the rounds.  The yardstick of a masked width is the shipped pair interpolated linearly in the row width:
t(8) = t(n_sem 5), t(24) = t(n_sem 21).

    python scripts/bench_nsem.py [--rounds 5] [--calls 5] [--out profiles/nsem_render_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from selfocc_amd import synthetic as sy  # noqa: E402
from selfocc_amd.render import RaySet, SDFVolume, render_rays, render_rays_autograd  # noqa: E402

CLASSES = (5, 4, 11, 20, 21)
SHIPPED = (5, 21)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nsem_render_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nsem.py measures on the GPU"
    d = torch.device("cuda:0")
    train = sy.make_rays("cfg5")
    r_train = RaySet(img2lidar=train.img2lidar.to(d), nx=train.nx, ny=train.ny, sx=train.sx, sy=train.sy)
    r_eval = RaySet(img2lidar=train.img2lidar.to(d), nx=800, ny=450, sx=1600 / 800, sy=768 / 450)
    cfg = sy.make_render_config("cfg5")
    cfg_b = sy.make_render_config("cfg5")
    cfg_b.bwd_scatter = 'binned'
    assert cfg.n_samples == 256 and r_train.n_rays == 28800 and r_eval.n_rays == 2160000

    vols, runs = {}, {}
    for n in CLASSES:
        v = sy.make_volume("cfg5", n_rgb=3, n_sem=n, seed=1)
        v.feat[..., 3 + n:] = 64.0                              # a pad channel may hold anything
        vols[n] = v.to(d)

    def bwd_call(n):
        v = vols[n]
        sdf, feat = v.sdf.clone().requires_grad_(True), v.feat.clone().requires_grad_(True)
        inv_s = torch.tensor([20.0], device=d, requires_grad=True)
        out = render_rays_autograd(SDFVolume(v.mapping, sdf, feat, 3, n), inv_s, r_train, cfg_b)
        loss = out['depth'].mean() + out['rgb'].mean() + out['sem'].square().mean() + out['sdf'].abs().mean()
        return loss

    for n in CLASSES:
        runs[('eval', n)] = lambda n=n: render_rays(vols[n], r_eval, cfg)
        runs[('train_fwd', n)] = lambda n=n: render_rays(vols[n], r_train, cfg, per_sample=True, want_grad_samples=True)

    def time_call(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    def time_bwd(n, calls):
        tot = 0.0
        for _ in range(calls):
            loss = bwd_call(n)                                  # the forward is outside the timed window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            loss.backward()
            e1.record()
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1)
        return tot / calls

    samples = {k: [] for k in list(runs) + [('bwd', n) for n in CLASSES]}
    for rnd in range(args.rounds + 1):                          # round 0 warms every shape up and is dropped
        for key, fn in runs.items():
            t = time_call(fn, args.calls if key[0] == 'train_fwd' else max(1, args.calls // 2))
            if rnd:
                samples[key].append(t)
        for n in CLASSES:
            t = time_bwd(n, max(1, args.calls // 2))
            if rnd:
                samples[('bwd', n)].append(t)

    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "unit": "ms per call", "rows": []}
    med = {k: statistics.median(v) for k, v in samples.items()}
    for what in ('eval', 'train_fwd', 'bwd'):
        for n in CLASSES:
            F = (3 + n + 3) & ~3
            row = dict(what=what, n_sem=n, row_floats=F, kernels='shipped' if n in SHIPPED else 'masked',
                       median_ms=round(med[(what, n)], 4), min_ms=round(min(samples[(what, n)]), 4), max_ms=round(max(samples[(what, n)]), 4))
            if n not in SHIPPED:
                lo, hi = med[(what, 5)], med[(what, 21)]
                yard = lo + (hi - lo) * (F - 8) / 16.0
                row.update(yardstick_ms=round(yard, 4), over_yardstick=round(med[(what, n)] / yard, 4))
            res["rows"].append(row)
            print(json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
