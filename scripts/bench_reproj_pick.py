"""Time the arg-max pick of the sdf_loss term (selfocc_reproj_pick_fwd / _bwd) against what the term would cost
without it, in ONE process, at the kitti_raw_depth training shape (scripts/shipped_cfg/kitti_raw_depth.json: one camera,
ray_number rays x num_samples samples, the loss's img_size).

Two routes, alternated inside every round, forward + backward each:
  (a) pick     reproj_pick: one launch for both temporal frames (4 values written per ray), and its backward: one pass that
               writes the dense (R, S) gradient of the per-sample values
  (b) wnorm    the normalised weights of each frame materialised by selfocc_reproj_fwd (`wnorm`, the other frame invalid: the
               launch the mono loss already makes, here with the (R, S) output on), torch.argmax, torch.gather, and for the
               backward torch.zeros + index_put(accumulate=True)
A figure is the median over the warm rounds of the device-event time of one forward + backward (min - max beside it); the
garbage collector is off while rounds run.  `disagree` = (ray, frame) pairs on which the two routes name another sample.

    python scripts/bench_reproj_pick.py [--rounds 20] [--out profiles/reproj_pick_bench.jsonl]
"""
import argparse
import gc
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from selfocc_amd import abi  # noqa: E402
from selfocc_amd._lib import check, current_stream, lib, ptr  # noqa: E402
from selfocc_amd.reproj import reproj_pick  # noqa: E402


def make_inputs(ny, nx, S, img_h, img_w, with_deltas, d):
    g = torch.Generator().manual_seed(0)
    R = ny * nx
    f = 0.6 * img_w
    K = np.array([[f, 0, img_w / 2, 0], [0, f, img_h / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])

    def motion(yaw_deg, tx, tz):
        y = np.deg2rad(yaw_deg)
        Rm = np.array([[np.cos(y), 0, np.sin(y), tx], [0, 1, 0, 0.02], [-np.sin(y), 0, np.cos(y), tz], [0, 0, 0, 1]])
        return torch.tensor(K @ Rm @ np.linalg.inv(K), dtype=torch.float32)
    xs = (torch.arange(nx, dtype=torch.float) + 0.5) * (img_w / nx)
    ys = (torch.arange(ny, dtype=torch.float) + 0.5) * (img_h / ny)
    pix = torch.stack([xs[None].expand(ny, -1), ys[:, None].expand(-1, nx)], -1).reshape(R, 2)
    near = torch.rand(R, 1, generator=g) * 0.5
    far = 10.0 + torch.rand(R, 1, generator=g) * 70.0
    edges = near + (far - near) * torch.linspace(0, 1, S + 1)[None]
    c = dict(weights=torch.softmax(torch.randn(R, S, generator=g) * 3, -1) * torch.rand(R, 1, generator=g),
             ts=(edges[:, :-1] + edges[:, 1:]) / 2, deltas=(edges[:, 1:] - edges[:, :-1]) if with_deltas else None,
             values=0.3 * torch.randn(R, S, generator=g), pix=pix, T_prev=motion(1.5, 0.1, -0.8), T_next=motion(-1.5, -0.1, 0.8),
             g=torch.randn(R, 2, generator=g), img=torch.rand(3, int(img_h), int(img_w), generator=g),
             rgb=torch.rand(R, 3, generator=g), invalid=torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0])))
    return {k: (None if v is None else v.contiguous().to(d)) for k, v in c.items()}


def wnorm_route(c, img_h, img_w):
    R, S = c['weights'].shape
    picks = []
    for Ts in ((c['T_prev'], c['invalid']), (c['invalid'], c['T_next'])):
        a = abi.SoReprojArgs()
        a.weights, a.ts, a.deltas = ptr(c['weights']), ptr(c['ts']), ptr(c['deltas'])
        a.pix, a.curr_rgb = ptr(c['pix']), ptr(c['rgb'])
        a.T_prev, a.T_next = ptr(Ts[0]), ptr(Ts[1])
        a.img_prev, a.img_next = ptr(c['img']), ptr(c['img'])
        a.R, a.S, a.Hi, a.Wi, a.img_h, a.img_w = R, S, c['img'].shape[1], c['img'].shape[2], float(img_h), float(img_w)
        wn = torch.empty(R, S, device=c['weights'].device)
        l1, comb, anyv = torch.empty(R, device=wn.device), torch.empty(R, 3, device=wn.device), torch.empty(R, device=wn.device)
        a.wnorm, a.l1, a.rgb_combine, a.any_valid = ptr(wn), ptr(l1), ptr(comb), ptr(anyv)
        check(lib().selfocc_reproj_fwd(a, current_stream(wn.device)), "selfocc_reproj_fwd")
        picks.append(wn.argmax(dim=1))
    idx = torch.stack(picks, 1)
    val = torch.gather(c['values'], 1, idx)
    rows = torch.arange(R, device=idx.device)[:, None].expand(-1, 2)
    grad = torch.zeros(R, S, device=idx.device).index_put((rows, idx), c['g'], accumulate=True)
    return val, idx, grad


def pick_route(c, img_h, img_w):
    values = c['values'].detach().requires_grad_(True)
    val, idx = reproj_pick(values, c['weights'], c['ts'], c['deltas'], c['pix'], c['T_prev'], c['T_next'], img_h, img_w)
    grad, = torch.autograd.grad(val, values, c['g'])
    return val.detach(), idx, grad


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cfg", default=os.path.join(ROOT, "scripts", "shipped_cfg", "kitti_raw_depth.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproj_pick_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_reproj_pick.py measures on the GPU"
    d = torch.device("cuda:0")
    cfg = json.load(open(args.cfg))
    head = cfg['model']['head']
    (ny, nx), S = head['ray_number'], head['num_samples']
    img_h, img_w = next(l for l in cfg['loss']['loss_cfgs'] if l['type'] == 'ReprojLossMonoMultiNew')['img_size']
    lines = []
    for with_deltas in (False, True):
        c = make_inputs(ny, nx, S, img_h, img_w, with_deltas, d)
        variants = {'pick': lambda: pick_route(c, img_h, img_w), 'wnorm': lambda: wnorm_route(c, img_h, img_w)}
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
        (va, ia, ga), (vb, ib, gb) = variants['pick'](), variants['wnorm']()
        torch.cuda.synchronize()
        disagree = int((ia != ib).sum())
        res = dict(cfg=os.path.basename(args.cfg), n_rays=ny * nx, n_samples=S, img_size=[img_h, img_w], deltas=with_deltas,
                   rounds=args.rounds, warmup=args.warmup, gpu=torch.cuda.get_device_name(0), disagree=disagree,
                   grad_equal=bool(torch.equal(ga, gb)) if disagree == 0 else None,
                   picks_not_zero_share=round(float((ia > 0).float().mean()), 4))
        for k, v in times.items():
            res[f'{k}_ms'] = round(statistics.median(v), 4)
            res[f'{k}_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
        res['wnorm_over_pick'] = round(res['wnorm_ms'] / res['pick_ms'], 2)
        print(json.dumps(res), flush=True)
        lines.append(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
