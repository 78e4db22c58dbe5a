#!/usr/bin/env python
"""Generate tests/golden/depth_metric.npz by running the REAL reference DepthMetric._after_step and
compute_depth_errors_torch (utils/metric_util.py, loaded by file path from the read-only reference tree with the
stand-ins of make_golden.install_stubs) on three seeded synthetic frames, on CPU.

Frame: 6 cameras, a 45 x 80 rendered depth image, n = 3 000 LiDAR points per camera, loc ~ U(-0.05, 1.05) (border
clamping), about 30 % of the points valid.  Camera 1 has an even valid count, camera 2 tied values (quantised gt, a
piecewise-constant image), camera 3 a single valid point; camera 4 has depths beyond 80 m and below 1e-3 m (the clamp).
No valid point has thresh = max(gt / p, p / gt) within 1e-4 relative of 1.25, 1.25^2 or 1.25^3 for either eval type
(the gt of such a point is nudged and the frame re-checked), so a1-a3 are exact even though CPU and GPU grid_sample
may differ in the last bit.  The buffers are read directly (``_after_epoch`` needs torch.distributed).

Run:  python tests/golden/make_golden_depth_metric.py        (needs the reference tree; ~2 s)
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402

N, H, W, NPTS = 6, 45, 80, 3000
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
BUFFERS = ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3', 'scaling', 'count')


def sampled(pred, loc):
    return F.grid_sample(pred.unsqueeze(1), loc.unsqueeze(1) * 2 - 1, mode='bilinear', padding_mode='border',
                         align_corners=True).reshape(N, -1)


def near_threshold(gt, p):
    """bool (n): thresh of the reference (f32, after the clamp) within 1e-4 relative of a threshold"""
    p = torch.clamp(p, 1e-3, 80)
    th = torch.maximum(gt / p, p / gt).double()
    return torch.stack([(th / t - 1).abs() < 1e-4 for t in THRESHOLDS]).any(0)


def make_frame(g):
    pred = torch.rand(N, H, W, generator=g) * 50 + 1.0
    pred[2] = (pred[2] / 8).floor() * 8 + 1                         # piecewise-constant: tied samples
    pred[4, :5] = 95.0                                              # beyond the 80 m clamp
    pred[4, -5:] = 1e-4                                             # below the 1e-3 clamp
    loc = torch.rand(N, NPTS, 2, generator=g) * 1.1 - 0.05
    loc[:, :8] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [0.5, 0.0], [0.0, 0.5],
                               [1.0, 0.5], [0.5, 1.0]])             # exactly on the image edges / corners
    mask = torch.rand(N, NPTS, generator=g) < 0.3
    mask[:, :8] = True
    mask[3] = False
    mask[3, 123] = True                                             # one valid point
    if int(mask[1].sum()) % 2:
        mask[1, torch.nonzero(~mask[1])[0, 0]] = True               # even count
    gt = torch.rand(N, NPTS, generator=g) * 60 + 0.5
    gt[2] = (gt[2] / 4).floor() * 4 + 2                             # tied gt values
    p = sampled(pred, loc)
    for _ in range(50):                                             # keep every valid thresh clear of 1.25^k
        bad = torch.zeros(N, NPTS, dtype=torch.bool)
        for c in range(N):
            m = mask[c]
            scale = torch.median(gt[c][m]) / torch.median(p[c][m])
            for q in (p[c], scale * p[c]):
                bad[c] |= m & near_threshold(gt[c], q)
        if not bad.any():
            return pred, loc, gt, mask
        gt[bad] *= 1.003
    raise RuntimeError("could not keep the thresholds clear")


def main():
    assert os.path.isdir(REF), f"{REF} not found: golden vectors can only be regenerated where the reference is mounted"
    install_stubs()
    spec = importlib.util.spec_from_file_location('ref_metric_util', os.path.join(REF, 'utils', 'metric_util.py'))
    mu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mu)
    g = torch.Generator().manual_seed(20241008)
    names = [f'cam{i}' for i in range(N)]
    metric = mu.DepthMetric(camera_names=names, eval_types=['raw', 'median'])
    frames = [make_frame(g) for _ in range(3)]
    out = {}
    for k, (pred, loc, gt, mask) in enumerate(frames):
        metric._after_step(loc.clone(), gt.clone(), mask.clone(), pred.clone())
        p = sampled(pred, loc)
        rows = [torch.stack(mu.compute_depth_errors_torch(gt[c][mask[c]].clone(), p[c][mask[c]].clone()))
                for c in range(N)]
        out[f'f{k}.pred'], out[f'f{k}.loc'], out[f'f{k}.gt'] = pred.numpy(), loc.numpy(), gt.numpy()
        out[f'f{k}.mask'] = mask.numpy()
        out[f'f{k}.errors'] = torch.stack(rows).numpy()
        for name in BUFFERS:
            out[f'after{k}.{name}'] = getattr(metric, name).detach().clone().numpy()
    for name in BUFFERS:
        out[name] = getattr(metric, name).numpy()
    path = os.path.join(HERE, 'depth_metric.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, keys={len(out)}")


if __name__ == '__main__':
    main()
