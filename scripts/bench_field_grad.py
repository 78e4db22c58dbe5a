#!/usr/bin/env python3
"""The SDF gradient at arbitrary points (selfocc_field_grad / selfocc_field_grad_bwd) against its two
yardsticks, on the nuscenes_occ volume (257 x 257 x 25) with N = 262 144 uniform points:

  ops    field_grad_autograd, analytic and numerical (delta 0.01 m), forward and forward + backward, against the only way to get
         these numbers without it: render_rays_autograd on N one-sample explicit rays whose origins are the points (forward, and
         forward + backward of the per-sample `grad` / `sdf`).  The variants take turns, one timed iteration each per round, so
         that clock and cache drift hit all of them alike; the medians over the rounds are reported.
  train  the nuscenes_occ training iteration (scripts/hotpath_common.py) with use_uniform_gradient off (the shipped config) and
         on (nbr_gradient_points = N, sample_gradient as shipped, analytic and delta 0.01), again in turns; `spread` is the
         knob-off iteration's own (max - min) / median over the rounds.

``--package-root DIR`` imports selfocc_amd and hotpath_common from another checkout (the parent commit, built there): with
``--only train_off`` that measures the parent's iteration on the same box for the A/B of the knob-off path.

One JSON line per section on stdout, appended to --out.

usage: python scripts/bench_field_grad.py [--rounds 30] [--warmup 3] [--n 262144] [--only ops train] [--label this]
                                          [--package-root DIR] [--out profiles/field_grad_bench.jsonl]"""
import argparse
import gc
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=262144)
ap.add_argument("--delta", type=float, default=0.01)
ap.add_argument("--only", nargs="+", default=["ops", "train"], choices=["ops", "train", "train_off"])
ap.add_argument("--label", default="this")
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=os.path.join("profiles", "field_grad_bench.jsonl"))
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.package_root, "scripts"))
sys.path.insert(0, args.package_root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

D0 = torch.device("cuda:0")


def take_turns(variants, rounds, warmup):
    """{name: [ms per round]}: every round runs each variant once, in order, between two events of its own"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    gc.collect()
    gc.disable()
    try:
        for _ in range(rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
    finally:
        gc.enable()
    return times


def summary(times):
    out = {}
    for k, t in times.items():
        out[f"{k}_ms"] = round(statistics.median(t), 4)
        out[f"{k}_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
    return out


def bench_ops():
    from selfocc_amd import abi, synthetic as sy
    from selfocc_amd.occ import field_grad, field_grad_autograd
    from selfocc_amd.render import RaySet, RenderConfig, SDFVolume, render_rays_autograd
    vol = sy.make_volume("cfg5").to(D0)                        # the shipped nuscenes_occ volume: 257 x 257 x 25
    aabb = sy.CONFIGS["cfg5"]["aabb"]
    n = args.n
    g = torch.Generator(device='cpu').manual_seed(0)
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    pts = (lo + torch.rand(n, 3, generator=g) * (hi - lo)).to(D0).contiguous()
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).to(D0).contiguous()
    g_grad, g_sdf = torch.randn(n, 3, generator=g).to(D0), torch.randn(n, generator=g).to(D0)
    sdf_p = vol.sdf.clone().requires_grad_(True)
    v = SDFVolume(vol.mapping, sdf_p, None, 0, 0)
    inv_s = torch.tensor([20.0], device=D0)
    rays = RaySet(origins=pts, dirs=dirs, dir_norm=None)
    cfg = RenderConfig(aabb=aabb, n_samples=1, near_plane=0.0, sample_pos=abi.SAMPLE_AT_START, jitter_mode=abi.JITTER_NONE)

    def both(q):
        sdf_p.grad = None
        ((q['grad'] * g_grad[:, None] if q['grad'].dim() == 3 else q['grad'] * g_grad).sum()
         + (q['sdf'].reshape(-1) * g_sdf).sum()).backward()

    def render():
        return render_rays_autograd(v, inv_s, rays, cfg, want_grad_samples=True)

    variants = {
        "analytic_fwd": lambda: field_grad(vol, pts),
        "numerical_fwd": lambda: field_grad(vol, pts, 'numerical', args.delta),
        "render_rays_fwd": lambda: render(),
        "analytic_fwd_bwd": lambda: both(field_grad_autograd(v, pts)),
        "numerical_fwd_bwd": lambda: both(field_grad_autograd(v, pts, 'numerical', args.delta)),
        "render_rays_fwd_bwd": lambda: both(render()),
    }
    # the three routes compute the same thing: the analytic gradient is the render's, bit for bit
    with torch.no_grad():
        assert torch.equal(field_grad(vol, pts)['grad'], render()['grad'][:, 0])
    res = dict(section="ops", label=args.label, volume=list(vol.sdf.shape), n=n, delta=args.delta, rounds=args.rounds,
               warmup=args.warmup, gpu=torch.cuda.get_device_name(0))
    res.update(summary(take_turns(variants, args.rounds, args.warmup)))
    for k in ("fwd", "fwd_bwd"):
        res[f"render_over_analytic_{k}"] = round(res[f"render_rays_{k}_ms"] / res[f"analytic_{k}_ms"], 2)
        res[f"numerical_over_analytic_{k}"] = round(res[f"numerical_{k}_ms"] / res[f"analytic_{k}_ms"], 2)
    return res


def bench_train(knob_on):
    import copy
    import hotpath_common as hc
    name = "nuscenes_occ"
    os.environ['eval'] = 'false'
    base = hc.shipped(name)
    heads = {"off": {}}
    if knob_on:
        heads["on_analytic"] = dict(use_uniform_gradient=True, nbr_gradient_points=args.n)
        heads["on_numerical"] = dict(use_uniform_gradient=True, nbr_gradient_points=args.n, uniform_gradient_delta=args.delta)
    runs, rows = {}, {}
    for key, kw in heads.items():
        cfg = copy.deepcopy(base)
        cfg['model']['head'].update(kw)
        torch.manual_seed(0)
        np.random.seed(0)
        mods = hc.build(cfg, D0, want_loss=True)
        for m in mods[:3]:
            m.train()
        fr = hc.frame_inputs(cfg, name, D0, seed=0)
        params = [p for m in mods[:3] for p in m.parameters()]

        def step(mods=mods, cfg=cfg, fr=fr, params=params, key=key):
            for p in params:
                p.grad = None
            _, _, out = hc.train_iteration(mods, cfg, fr, global_iter=1)
            rows[key] = out['eik_grad'].shape[0]
        runs[key] = step
    res = dict(section="train", label=args.label, config=name, n=args.n, delta=args.delta, rounds=args.rounds, warmup=args.warmup,
               gpu=torch.cuda.get_device_name(0))
    times = take_turns(runs, args.rounds, args.warmup)
    res.update(summary(times))
    res["eik_rows"] = rows
    res["off_spread"] = round((max(times["off"]) - min(times["off"])) / statistics.median(times["off"]), 4)
    for k in heads:
        if k != "off":
            res[f"{k}_minus_off_ms"] = round(res[f"{k}_ms"] - res["off_ms"], 4)
    return res


def main():
    lines = []
    if "ops" in args.only:
        lines.append(bench_ops())
        print(json.dumps(lines[-1]), flush=True)
    if "train" in args.only or "train_off" in args.only:
        lines.append(bench_train("train" in args.only))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fo:
        for res in lines:
            fo.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
