"""Time the per-sample reprojection term at other channel counts (selfocc_reproj_c_fwd / _bwd) against the
torch-op form of the same reference lines (tests/reproj_dims_port.py, run on the GPU), in ONE process, at the shipped nuScenes
training shape per camera: R = 4 800 rays (48 x 100 lattice) x S = 256 samples, img_size = [768, 1600].

Cases:  C = 3 through the 3-channel entry (selfocc_reproj_fwd, planar 768 x 1600 images: what dims == 3 runs),
        C = 3 through the channel-last entry on the same images (what the kernel's channel-last tap fetch costs beside its
        planar one; nothing is routed this way), C = 16 and C = 96 on 96 x 200 feature maps.
Per case, alternated inside every round: the kernel forward, the kernel forward + backward, the torch form forward, the torch
form forward + backward (autograd), and for the generic entry the two channel_last copies the loss makes once per camera and
call (the kernel figures are taken on images that are already channel-last).  A figure is the median over the warm rounds of the
device-event time of back-to-back calls (`--inner-kernel` of them for the kernel and copy rows, `--inner` for the torch form),
divided by their number (min - max beside it); the garbage collector is off while rounds run.  `max_abs_diff` = kernel against
the torch form (float32 both) on l1 / combine / the gradient: a sanity figure, the parity statement is
tests/test_reproj_dims_gpu.py.

    python scripts/bench_reproj_dims.py [--rounds 10] [--out profiles/reproj_dims_bench.jsonl]
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from reproj_dims_port import reproj_sample_port_c  # noqa: E402
from selfocc_amd.reproj import ReprojSampleCFunction, ReprojSampleFunction, channel_last  # noqa: E402


def make_inputs(ny, nx, S, img_h, img_w, C, hw, d):
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
             ts=(edges[:, :-1] + edges[:, 1:]) / 2, pix=pix, curr=torch.rand(R, C, generator=g),
             T_prev=motion(1.5, 0.1, -0.8), T_next=motion(-1.5, -0.1, 0.8),
             img_prev=torch.rand(C, *hw, generator=g), img_next=torch.rand(C, *hw, generator=g),
             g_l1=torch.randn(R, generator=g), g_comb=torch.randn(R, C, generator=g))
    return {k: v.contiguous().to(d) for k, v in c.items()}


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--inner-kernel", type=int, default=100)
    ap.add_argument("--rays", type=int, nargs=2, default=[48, 100])
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--cases", type=int, nargs="*", default=[0, 1, 2, 3], help="which of the four cases to run, by position "
                    "(one per process under a kernel trace, whose statistics are per kernel name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproj_dims_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_reproj_dims.py measures on the GPU"
    d = torch.device("cuda:0")
    img_h, img_w = 768, 1600
    (ny, nx), S = args.rays, args.samples
    lines = []
    cases = (("reproj", 3, (768, 1600)), ("reproj_c", 3, (768, 1600)), ("reproj_c", 16, (96, 200)), ("reproj_c", 96, (96, 200)))
    for entry, C, hw in (cases[i] for i in args.cases):
        c = make_inputs(ny, nx, S, img_h, img_w, C, hw, d)
        generic = entry == "reproj_c"
        fn = ReprojSampleCFunction if generic else ReprojSampleFunction
        imgs = (channel_last(c['img_prev']), channel_last(c['img_next'])) if generic else (c['img_prev'], c['img_next'])

        def kernel(bwd):
            w = c['weights'].detach().requires_grad_(bwd)
            l1, comb, _ = fn.apply(w, c['ts'], None, c['pix'], c['curr'], c['T_prev'], c['T_next'], *imgs, img_h, img_w)
            grad = torch.autograd.grad([l1, comb], w, [c['g_l1'], c['g_comb']])[0] if bwd else None
            return l1.detach(), comb.detach(), grad

        def torch_form(bwd):
            w = c['weights'].detach().requires_grad_(bwd)
            with torch.set_grad_enabled(bwd):
                l1, comb, _ = reproj_sample_port_c(w, c['ts'], None, c['pix'], c['curr'], c['T_prev'], c['T_next'],
                                                   c['img_prev'], c['img_next'], img_h, img_w)
            grad = torch.autograd.grad([l1, comb], w, [c['g_l1'], c['g_comb']])[0] if bwd else None
            return l1.detach(), comb.detach(), grad

        variants = {'kernel_fwd': lambda: kernel(False), 'kernel_fwd_bwd': lambda: kernel(True),
                    'torch_fwd': lambda: torch_form(False), 'torch_fwd_bwd': lambda: torch_form(True)}
        if generic:
            variants['channel_last_x2'] = lambda: (channel_last(c['img_prev']), channel_last(c['img_next']))
        times = {k: [] for k in variants}
        gc.collect()
        gc.disable()
        try:
            for rnd in range(args.warmup + args.rounds):
                for k, v in variants.items():
                    ms = timed(v, args.inner if k.startswith('torch') else args.inner_kernel)
                    if rnd >= args.warmup:
                        times[k].append(ms)
        finally:
            gc.enable()
        (kl, kc, kg), (tl, tc, tg) = kernel(True), torch_form(True)
        torch.cuda.synchronize()
        res = dict(entry=entry, C=C, img=list(hw), n_rays=ny * nx, n_samples=S, img_size=[img_h, img_w], rounds=args.rounds,
                   warmup=args.warmup, inner=args.inner, inner_kernel=args.inner_kernel, gpu=torch.cuda.get_device_name(0),
                   max_abs_diff=dict(l1=float((kl - tl).abs().max()), combine=float((kc - tc).abs().max()),
                                     grad=float((kg - tg).abs().max()), grad_scale=float(tg.abs().max())))
        for k, v in times.items():
            res[f'{k}_ms'] = round(statistics.median(v), 4)
            res[f'{k}_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
        res['torch_over_kernel_fwd'] = round(res['torch_fwd_ms'] / res['kernel_fwd_ms'], 2)
        res['torch_over_kernel_fwd_bwd'] = round(res['torch_fwd_bwd_ms'] / res['kernel_fwd_bwd_ms'], 2)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del c, imgs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
