"""The depth-evaluation metric tail at nuscenes shape (6 cameras, 450 x 800 rendered depth, n = 34 720 LiDAR points per
camera, ~15 % valid): selfocc_amd.DepthMetric._after_step (one HIP launch, no host sync) against a torch restatement of
the reference's loop (utils/metric_util.py:311-349: grid_sample, per camera two boolean-mask indexings, torch.median,
cal_depth_metric's small ops, += into the buffers).

  tail  : median over --iters calls (cyclic GC collected before and held off, as scripts/bench_hotpath_all.py) of the
          wall time of one _after_step including the drain of the stream (the reference path syncs inside anyway), and
          of the device time of our launch (events);
  frame : the depth-evaluation frame (eval_depth.py:150-227: lifter, encoder, head.prepare, head.render, built from the
          shipped nuscenes_depth config like scripts/bench_hotpath_eval.py) followed by the metric tail, end to end
          (wall time to the drained stream), both paths.
Prints one JSON line.  Launch counts: run under `rocprofv3 --kernel-trace --stats` with `--path ours|ref --no-frame`
and divide the dispatches by --warm + --iters.
    python scripts/bench_depth_metric.py [--iters 50] [--frame-iters 10] [--path both|ours|ref] [--no-frame]"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--frame-iters", type=int, default=10)
ap.add_argument("--path", default="both", choices=["both", "ours", "ref"])
ap.add_argument("--no-frame", action="store_true")
args = ap.parse_args()
d = torch.device("cuda:0")
CAMS = [f'cam{i}' for i in range(6)]


class RefDepthMetric(torch.nn.Module):
    """the reference's DepthMetric._after_step loop restated (buffers as in metric_util.py:286-299)"""

    def __init__(self):
        super().__init__()
        for k in ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3', 'scaling'):
            self.register_buffer(k, torch.zeros(2, 6))
        self.register_buffer('count', torch.zeros(1))

    @staticmethod
    def cal(p, gt):
        p = torch.clamp(p, 1e-3, 80)
        th = torch.maximum((gt / p), (p / gt))
        return dict(a1=(th < 1.25).to(torch.float).mean(), a2=(th < 1.25 ** 2).to(torch.float).mean(),
                    a3=(th < 1.25 ** 3).to(torch.float).mean(), rmse=((gt - p) ** 2).mean() ** .5,
                    rmse_log=((torch.log(gt) - torch.log(p)) ** 2).mean() ** .5,
                    abs_rel=(torch.abs(gt - p) / gt).mean(), sq_rel=(((gt - p) ** 2) / gt).mean())

    def _after_step(self, loc, gt, mask, pred):
        N, n = gt.shape
        pred = F.grid_sample(pred.unsqueeze(1), loc.unsqueeze(1) * 2 - 1, mode='bilinear', padding_mode='border',
                             align_corners=True).reshape(N, n)
        for cam, (g, p, m) in enumerate(zip(gt, pred, mask)):
            gm, pm = g[m], p[m]
            for t, typ in enumerate(('raw', 'median')):
                if typ == 'raw':
                    pc = pm
                    self.scaling[t, cam] += 1.0
                else:
                    s = torch.median(gm) / torch.median(pm)
                    pc = s * pm
                    self.scaling[t, cam] += s
                for k, v in self.cal(pc, gm).items():
                    getattr(self, k)[t, cam] += v
        self.count += 1


def frame_inputs(seed):
    g = torch.Generator(device=d).manual_seed(seed)
    pred = torch.rand(6, 450, 800, generator=g, device=d) * 60 + 0.5
    loc = torch.rand(6, 34720, 2, generator=g, device=d)
    gt = torch.rand(6, 34720, generator=g, device=d) * 60 + 0.5
    mask = torch.rand(6, 34720, generator=g, device=d) < 0.15
    return loc, gt, mask, pred


def metric(path):
    from selfocc_amd import DepthMetric
    return (DepthMetric(CAMS) if path == 'ours' else RefDepthMetric()).to(d)


def time_tail(path):
    m = metric(path)
    inp = frame_inputs(0)
    wall, dev = [], []
    gc.collect(); gc.disable()
    try:
        for it in range(args.warm + args.iters):
            torch.cuda.synchronize()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            m._after_step(*inp)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if it >= args.warm:
                wall.append((t1 - t0) * 1e3); dev.append(e0.elapsed_time(e1))
    finally:
        gc.enable()
    return dict(wall_ms=round(float(np.median(wall)), 4), device_ms=round(float(np.median(dev)), 4))


def time_frame(paths):
    import hotpath_common as hc
    os.environ['eval'] = 'true'
    torch.manual_seed(0)
    cfg = hc.modify_for_eval(hc.shipped("nuscenes_depth"), 'nuscenes')
    lifter, encoder, head, _ = hc.build(cfg, d)
    for mod in (lifter, encoder, head):
        mod.eval()
    img = tuple(cfg['img_size'])
    c2w, l2i, K = hc.ring_cameras(6, img, 1266.0)
    metas = [dict(lidar2img=l2i, img2lidar=c2w, img_shape=img)]
    feats = hc.fpn_feats(6, cfg['model']['encoder']['embed_dims'], img, d)
    loc, gt, mask, _ = frame_inputs(1)
    res = {}
    with torch.no_grad():
        for path in paths:
            m = metric(path)
            ts = []
            gc.collect(); gc.disable()
            try:
                for it in range(2 + args.frame_iters):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rep = encoder(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
                    head.prepare(rep, metas)
                    out = head.render(metas, batch=90000)
                    depth = out['ms_depths'][0].reshape(6, 450, 800)     # eval_depth.py:180-200
                    m._after_step(loc, gt, mask, depth)
                    torch.cuda.synchronize()
                    if it >= 2:
                        ts.append((time.perf_counter() - t0) * 1e3)
            finally:
                gc.enable()
            res[path] = round(float(np.median(ts)), 3)
    return res


paths = ['ours', 'ref'] if args.path == 'both' else [args.path]
res = {'tail_' + p: time_tail(p) for p in paths}
if not args.no_frame:
    res['frame_plus_tail_ms'] = time_frame(paths)
res['shape'] = dict(cams=6, h=450, w=800, n=34720, valid=0.15, iters=args.iters)
print(json.dumps(res))
