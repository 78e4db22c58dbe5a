"""CameraAwareSE + flatten at the shipped nuScenes shape (B 1, N 6, C = M = 96, FPN levels 96x200 / 48x100 / 24x50 / 12x25 =
153 000 pixels, 58.75 MB of maps), in ONE process, variants alternated round-robin, CUDA-event times after warm-up:

  fused        selfocc_camera_se_flatten_fwd / _bwd behind CameraAwareSE.flatten (csrc/camera_se.hip)
  torch        the composition the reference runs: gate multiply + F.conv2d 1x1 per level, two broadcast adds per level, cat
               (CameraAwareSE.flatten_torch) — the yardstick: code that exists without the fused kernels
  flatten      today's camera_aware=False cost alone: _FlattenFeats (selfocc_flatten_feats forward, column sums backward) —
               the floor the option adds to

The gate (6 x 96 numbers through BatchNorm1d / MLP / sigmoid, torch ops in every variant) is inside every camera-aware time.
One JSON line per variant: forward / backward medians, min, max, the 10th-to-90th percentile range, and the achieved bytes/s on
the compulsory traffic (forward: read the maps + write value = 117.5 MB; backward: read g and the maps, write the map
gradients = 176.3 MB).  --width 192 times camera_aware_mid_channels = 192 (the 3x3 reduce_conv, a vendor convolution, is in
both camera-aware variants then).

Kernel times and names come from a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -o p -- python scripts/bench_camera_se.py --iters 3
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import numpy as np
from selfocc_amd.model.encoder import CameraAwareSE
from selfocc_amd.model.encoder.tpvformer import _FlattenFeats

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=30, help='timed rounds (after 3 warm-up rounds)')
ap.add_argument('--width', type=int, default=96, help='camera_aware_mid_channels')
ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
args = ap.parse_args()
d = torch.device('cuda:0')
B, N, C, M = 1, 6, 96, args.width
LEVELS = ((96, 200), (48, 100), (24, 50), (12, 25))
S = sum(h * w for h, w in LEVELS)


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def spread(times):
    """run-to-run spread: the 10th-to-90th percentile range (a rare host hiccup of milliseconds lands in `max_ms`, not here)"""
    t = sorted(times)
    return t[int(0.9 * (len(t) - 1) + 0.5)] - t[int(0.1 * (len(t) - 1) + 0.5)]


def summarise(times, nbytes):
    med = statistics.median(times)
    return dict(median_ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4),
                p10_p90_ms=round(spread(times), 4), gbytes_per_s=round(nbytes / med / 1e6, 1))


g = torch.Generator().manual_seed(0)
maps = [torch.randn(B, N, C, h, w, generator=g).to(d) for h, w in LEVELS]
gv = torch.randn(N, S, B, C, generator=g).to(d)
cams = torch.randn(N, C, generator=g).to(d).requires_grad_(True)
lvls = torch.randn(len(LEVELS), C, generator=g).to(d).requires_grad_(True)


def ring_metas():
    """six pinholes around the ego origin: `intrinsic` and the camera-to-ego pose `cam2ego`"""
    Ks, Es = [], []
    for n in range(N):
        yaw = 2.0 * np.pi * n / N
        K = np.eye(4); K[0, 0] = K[1, 1] = 1260.0 + 5.0 * n; K[0, 2], K[1, 2] = 800.0 + n, 450.0 - n
        E = np.eye(4)
        E[:3, :3] = [[np.cos(yaw), 0.0, np.sin(yaw)], [np.sin(yaw), 0.0, -np.cos(yaw)], [0.0, 1.0, 0.0]]
        E[:3, 3] = [0.8 + 0.1 * n, 0.05 * n, 1.5]
        Ks.append(K); Es.append(E)
    return [dict(intrinsic=Ks, cam2ego=Es)]


metas = ring_metas()
torch.manual_seed(1)
mod = CameraAwareSE(C, M, C).to(d).train()          # training mode: BatchNorm1d normalises with the rig's own statistics

VARIANTS = {
    'fused': lambda xs: mod.flatten(xs, metas, cams, lvls),
    'torch': lambda xs: mod.flatten_torch(xs, metas, cams, lvls),
    'flatten': lambda xs: _FlattenFeats.apply(cams, lvls, *xs),
}
FWD_BYTES = 4 * (B * N * C * S + N * S * B * C)
BWD_BYTES = 4 * (N * S * B * C + 2 * B * N * C * S)
times = {k: dict(fwd=[], bwd=[]) for k in VARIANTS}
check = {}
for it in range(3 + args.iters):
    for k, fn in VARIANTS.items():
        xs = [m.detach().requires_grad_(True) for m in maps]
        e0 = ev()
        val = fn(xs)
        e1 = ev()
        val.backward(gv)
        e2 = ev()
        torch.cuda.synchronize()
        check[k] = (round(float(val.detach().double().mean()), 6), round(float(xs[0].grad.double().abs().mean()), 6))
        mod.zero_grad(); cams.grad = None; lvls.grad = None
        if it >= 3:
            times[k]['fwd'].append(e0.elapsed_time(e1))
            times[k]['bwd'].append(e1.elapsed_time(e2))
lines = []
for k in VARIANTS:
    rec = dict(shape=f'B {B} N {N} C {C} M {M} levels {list(LEVELS)}', variant=k, iters=args.iters, value_mean=check[k][0],
               dmap0_absmean=check[k][1], forward=summarise(times[k]['fwd'], FWD_BYTES), backward=summarise(times[k]['bwd'], BWD_BYTES))
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
verdict = {}
for direction in ('fwd', 'bwd'):
    f, t = times['fused'][direction], times['torch'][direction]
    gain = statistics.median(t) - statistics.median(f)
    noise = max(spread(f), spread(t))
    verdict[direction] = dict(torch_minus_fused_ms=round(gain, 4), run_to_run_spread_ms=round(noise, 4), fused_wins=bool(gain > noise))
lines.append(json.dumps(dict(verdict=verdict)))
print(lines[-1], flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write("\n".join(lines) + "\n")
