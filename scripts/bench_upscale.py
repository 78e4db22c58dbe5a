"""The 'linear_upscale' mapping against the shipped linear one, in ONE process: the nuScenes depth-evaluation frame
(eval_depth.py: 6 x 450 x 800 = 2.16 M rays x 256 samples, render stage) and the nuscenes_occ training iteration, each built
from the shipped config and from its upscale variant (hotpath_common.upscale_variant: NeuSHead's default mapping_args,
321 x 321 x 31).  Medians of CUDA-event times over warm runs; JSON per variant.  The render kernels' own times come from a
separate rocprofv3 run of the same script:
    rocprofv3 --kernel-trace --stats -d <dir> -o p -- python scripts/bench_upscale.py --iters 2
The upscale route is the canonical march (no affine stepping, no brick re-pack, no skip codes), so its render stage is
expected to be slower than the linear fast path."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import hotpath_common as hc

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=7, help='timed runs per variant (after 2 warm-up runs)')
ap.add_argument('--only', choices=['eval', 'train', 'both'], default='both')
args = ap.parse_args()
d = torch.device('cuda:0')


def med(v):
    return round(statistics.median(v), 3)


def eval_frame(upscale):
    os.environ['eval'] = 'true'
    cfg = hc.shipped_for_eval('nuscenes_depth')
    if upscale:
        cfg = hc.upscale_variant(cfg)
    torch.manual_seed(0)
    mods = hc.build(cfg, d)
    for m in mods[:3]:
        m.eval()
    lifter, encoder, head = mods[:3]
    fr = hc.frame_inputs(cfg, 'nuscenes_depth', d, seed=0, want_images=False)
    metas, feats, _ = fr
    st = {}
    with torch.no_grad():
        for it in range(2 + args.iters):
            e0 = hc.ev()
            rep = encoder(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
            e1 = hc.ev()
            head.prepare(rep, metas)
            e2 = hc.ev()
            out = head.render(metas, batch=90000)
            e3 = hc.ev()
            torch.cuda.synchronize()
            if it >= 2:
                for k, (a, b) in dict(encoder_fwd=(e0, e1), prepare_volume=(e1, e2), render=(e2, e3)).items():
                    st.setdefault(k, []).append(a.elapsed_time(b))
    res = {k: med(v) for k, v in st.items()}
    res.update(frame='nuscenes_depth eval', mapping='linear_upscale' if upscale else 'linear (shipped)',
               lattice=[head.model.field.size_h, head.model.field.size_w, head.model.field.size_d],
               n_rays=int(out['ms_depths'][0].numel()), samples=cfg['model']['head']['num_samples'],
               depth_mean=round(float(out['ms_depths'][0].mean()), 3))
    del mods, lifter, encoder, head, out
    torch.cuda.empty_cache()
    return res


def train_iter(upscale):
    os.environ['eval'] = 'false'
    cfg = hc.shipped('nuscenes_occ')
    if upscale:
        cfg = hc.upscale_variant(cfg)
    torch.manual_seed(0)
    np.random.seed(0)
    mods = hc.build(cfg, d, want_loss=True)
    for m in mods[:3]:
        m.train()
    head = mods[2]
    params = [p for m in mods[:3] for p in m.parameters()]
    fr = hc.frame_inputs(cfg, 'nuscenes_occ', d, seed=0)
    st = {}
    for it in range(2 + args.iters):
        for p in params:
            p.grad = None
        ev = {}
        hc.train_iteration(mods, cfg, fr, global_iter=it, events=ev)
        torch.cuda.synchronize()
        if it >= 2:
            for k, (a, b) in dict(encoder_fwd=('t0', 't1'), head_fwd=('t1', 't2'), losses_fwd=('t2', 't3'),
                                  backward_all=('t3', 't4'), iteration=('t0', 't4')).items():
                st.setdefault(k, []).append(ev[a].elapsed_time(ev[b]))
    res = {k: med(v) for k, v in st.items()}
    res.update(frame='nuscenes_occ training iteration', mapping='linear_upscale' if upscale else 'linear (shipped)',
               lattice=[head.model.field.size_h, head.model.field.size_w, head.model.field.size_d],
               rays=cfg['num_rays'][0] * cfg['num_rays'][1] * cfg['model']['encoder']['num_cams'],
               samples=cfg['model']['head']['num_samples'])
    del mods, head, params
    torch.cuda.empty_cache()
    return res


if args.only in ('eval', 'both'):
    for up in (False, True):
        print(json.dumps(eval_frame(up)), flush=True)
if args.only in ('train', 'both'):
    for up in (False, True):
        print(json.dumps(train_iter(up)), flush=True)
