"""View-dependent colour (spherical harmonics, sh_deg 1 / 2) against the shipped degree-0 launches, in ONE process, at the
render operator: variants alternated round-robin, medians of CUDA-event times after warm-up, one JSON line per variant.

  eval   the nuScenes novel-view / depth evaluation lattice, 6 x 450 x 800 = 2.16 M pixel-grid rays x 256 samples, on the
         257 x 257 x 25 nuscenes_occ volume: sdf + rgb as shipped (degree 0, 4-float rows, fast march), the shipped 3 + 21
         channel launch (24-float rows: the yardstick for the 28-float rows of degree 2), degree 1 / 2 (relu), degree 2 (sigmoid)
  train  the nuscenes_occ training lattice, 6 x 48 x 100 rays x 256 samples, single jitter, random background:
         render forward (per-sample outputs) + backward through render_rays_autograd, the same variants

Kernel times and names come from a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -o p -- python scripts/bench_sh.py --iters 2
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from selfocc_amd import abi, synthetic as sy
from selfocc_amd.render import RaySet, render_rays, render_rays_autograd

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=7, help='timed rounds (after 2 warm-up rounds)')
ap.add_argument('--only', choices=['eval', 'train', 'both'], default='both')
ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
args = ap.parse_args()
d = torch.device('cuda:0')

# name -> make_volume keywords
VARIANTS = {
    'deg0 rgb (shipped, 4 floats)': dict(n_rgb=3),
    'deg0 rgb + 21 sem (shipped, 24 floats)': dict(n_rgb=3, n_sem=21),
    'deg1 relu (12 floats)': dict(n_rgb=3, sh_deg=1),
    'deg2 relu (28 floats)': dict(n_rgb=3, sh_deg=2),
    'deg2 sigmoid (28 floats)': dict(n_rgb=3, sh_deg=2, sh_act='sigmoid'),
    'deg0 sigmoid (4 floats)': dict(n_rgb=3, sh_act='sigmoid'),
}


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def summarise(times):
    return dict(median_ms=round(statistics.median(times), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3))


def run(kind):
    vols = {k: sy.make_volume("cfg5", seed=0, **kw).to(d) for k, kw in VARIANTS.items()}
    cams = sy.make_cameras("cfg5", 0).to(d)
    if kind == 'eval':
        rays = RaySet(img2lidar=cams, nx=800, ny=450, sx=2.0, sy=768 / 450)
        cfg = sy.make_render_config("cfg5", inv_s=20.0, bkgd_mode=abi.BKGD_CONST, bkgd=(1.0, 1.0, 1.0), clamp_rgb=True)
    else:
        r = sy.make_rays("cfg5")
        rays = RaySet(img2lidar=cams, nx=r.nx, ny=r.ny, sx=r.sx, sy=r.sy)
        cfg = sy.make_render_config("cfg5", inv_s=20.0, jitter_mode=abi.JITTER_SINGLE, bkgd_mode=abi.BKGD_PER_RAY)
    N = rays.n_rays
    g = torch.Generator(device=d).manual_seed(1)
    t_rand, bk = torch.rand(N, generator=g, device=d), torch.rand(N, 3, generator=g, device=d)
    G = torch.randn(N, 3, generator=g, device=d)
    times = {k: {} for k in vols}
    check = {}
    for it in range(2 + args.iters):
        for k, v in vols.items():
            if kind == 'eval':
                e0 = ev()
                out = render_rays(v, rays, cfg)
                e1 = ev()
                torch.cuda.synchronize()
                t = dict(render_fwd=e0.elapsed_time(e1))
            else:
                sdf, feat = v.sdf.detach().requires_grad_(True), v.feat.detach().requires_grad_(True)
                inv_s = torch.tensor([cfg.inv_s], device=d, requires_grad=True)
                e0 = ev()
                out = render_rays_autograd(v.with_tensors(sdf, feat), inv_s, rays, cfg, t_rand=t_rand, bkgd_rays=bk)
                e1 = ev()
                loss = (out['rgb'] * G).sum() + out['depth'].sum() + (out['grad'].norm(dim=-1) - 1).square().mean()
                e2 = ev()
                loss.backward()
                e3 = ev()
                torch.cuda.synchronize()
                t = dict(render_fwd=e0.elapsed_time(e1), backward_all=e2.elapsed_time(e3))
            check[k] = round(float(out['rgb'].detach().mean()), 5)
            if it >= 2:
                for n, x in t.items():
                    times[k].setdefault(n, []).append(x)
    lines = []
    for k in vols:
        rec = dict(shape='eval 6x450x800 rays x 256 samples, 257x257x25' if kind == 'eval' else 'train 6x48x100 rays x 256 samples, 257x257x25',
                   variant=k, n_rays=N, rgb_mean=check[k], **{n: summarise(x) for n, x in times[k].items()})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    return lines


all_lines = []
if args.only in ('eval', 'both'):
    all_lines += run('eval')
if args.only in ('train', 'both'):
    all_lines += run('train')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write("\n".join(all_lines) + "\n")
