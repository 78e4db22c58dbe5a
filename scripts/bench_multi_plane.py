"""The per-plane norm / FFN steps of TPVFormerLayer(multi_plane_ffn_norm=True) at the nuscenes_occ plane sizes (257 x 257 x 25:
66 049 / 6 425 / 6 425 rows, 96 dims, FFN width 192), in ONE process, variants alternated round-robin after warm-up, garbage
collector off, CUDA-event times:

  norm step   (a) shared      FastLayerNorm on the concatenated 78 899 rows (selfocc_layernorm_fwd / _bwd): existing code
              (b) grouped     MultiPlaneNorm.forward_cat: ONE selfocc_layernorm_*_grouped launch per direction
              (c) per_plane   the per-plane composition of the existing kernels: three FastLayerNorm calls + the cat
  ffn step    (a) shared      FFN on the concatenated rows
              (b) grouped     MultiPlaneFFN.forward_cat: the grouped tall-Linear kernels, one launch per Linear and direction
              (c) per_plane   MultiPlaneFFN on the split planes: one FFN per plane (the existing kernels) + the cat
each in inference (no_grad forward) and training (forward + backward) mode.  `--repeats` blocks of `--iters` rounds: a variant's
time is the median over all rounds, the spread of (a) is (max - min) / median over the blocks' medians.  Then one whole encoder
inference frame and one training step (forward + backward of a seeded scalar) of the shipped nuscenes_occ encoder with and
without multi_plane_ffn_norm, built through scripts/hotpath_common.py.  One JSON line per measurement.

Kernel times and names come from a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -o p -- python scripts/bench_multi_plane.py --iters 3 --repeats 1 --no-encoder
"""
import argparse
import copy
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

import hotpath_common as hc
from selfocc_amd.model import bricks

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=20, help='timed rounds per block (after 3 warm-up rounds)')
ap.add_argument('--repeats', type=int, default=5, help='blocks')
ap.add_argument('--no-encoder', action='store_true', help='skip the whole-encoder frames')
ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
args = ap.parse_args()
d = torch.device('cuda:0')
SIZES, C, FF = [257 * 257, 25 * 257, 257 * 25], 96, 192
T = sum(SIZES)
lines = []


def emit(rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def timed(fn):
    e0 = hc.ev()
    fn()
    e1 = hc.ev()
    return e0, e1


def measure(variants):
    """{name: [[ms of block 0], [ms of block 1], ...]} with the variants alternated inside every round"""
    times = {k: [] for k in variants}
    for _ in range(3):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        block = {k: [] for k in variants}
        for _ in range(args.iters):
            evs = {k: timed(fn) for k, fn in variants.items()}
            torch.cuda.synchronize()
            for k, (e0, e1) in evs.items():
                block[k].append(e0.elapsed_time(e1))
        for k in variants:
            times[k].append(block[k])
    return times


def summarise(blocks):
    flat = [t for b in blocks for t in b]
    meds = [statistics.median(b) for b in blocks]
    med = statistics.median(flat)
    return dict(median_ms=round(med, 4), min_ms=round(min(flat), 4), max_ms=round(max(flat), 4),
                block_medians_ms=[round(m, 4) for m in meds], block_spread=round((max(meds) - min(meds)) / med, 4))


g = torch.Generator().manual_seed(0)
x = torch.randn(1, T, C, generator=g).to(d)
dy = torch.randn(1, T, C, generator=g).to(d)
torch.manual_seed(1)
shared_ln = bricks.FastLayerNorm(C).to(d)
mp_ln = bricks.MultiPlaneNorm(C).to(d)
pp_ln = bricks.MultiPlaneNorm(C).to(d)               # (c): the same module with the grouped route switched off per call
shared_ffn = bricks.FFN(C, FF, ffn_drop=0.1).to(d)
mp_ffn = bricks.MultiPlaneFFN(C, FF, ffn_drop=0.1).to(d)


def per_plane_ln(t):
    old, bricks.GROUPED_LN = bricks.GROUPED_LN, False
    try:
        return pp_ln.forward_cat(t, SIZES)
    finally:
        bricks.GROUPED_LN = old


def per_plane_ffn(t):
    return torch.cat(mp_ffn(torch.split(t, SIZES, 1)), 1)


def fwd(fn):
    def run():
        with torch.no_grad():
            fn(x)
    return run


def fwd_bwd(fn, params):
    params = list(params)
    xr = x.clone().requires_grad_(True)

    def run():
        torch.autograd.grad(fn(xr), [xr] + params, dy)
    return run


gc.disable()
STEPS = {
    'norm': dict(shared=(shared_ln, shared_ln), grouped=(lambda t: mp_ln.forward_cat(t, SIZES), mp_ln), per_plane=(per_plane_ln, pp_ln)),
    'ffn': dict(shared=(shared_ffn, shared_ffn), grouped=(lambda t: mp_ffn.forward_cat(t, SIZES), mp_ffn),
                per_plane=(per_plane_ffn, mp_ffn)),
}
for step, variants in STEPS.items():
    for mode in ('inference', 'training'):
        for m in {v[1] for v in variants.values()}:
            m.train(mode == 'training')
        fns = {k: (fwd(fn) if mode == 'inference' else fwd_bwd(fn, mod.parameters())) for k, (fn, mod) in variants.items()}
        res = {k: summarise(v) for k, v in measure(fns).items()}
        rec = dict(step=step, mode=mode, rows=SIZES, dims=[C, FF], iters=args.iters, repeats=args.repeats, **res)
        a, c = res['shared'], res['per_plane']
        if 'grouped' in res:
            b = res['grouped']
            rec['verdict'] = dict(grouped_beats_per_plane=bool(b['median_ms'] < c['median_ms']),
                                  grouped_over_shared=round(b['median_ms'] / a['median_ms'], 4),
                                  within_5pct_plus_spread_of_shared=bool(b['median_ms'] <= a['median_ms'] * (1.05 + a['block_spread'])))
        emit(rec)

if not args.no_encoder:
    base = hc.shipped('nuscenes_occ')
    mp_cfg = copy.deepcopy(base)
    for layer in mp_cfg['model']['encoder']['transformerlayers']:
        ff, drop = layer.pop('feedforward_channels'), layer.pop('ffn_dropout')
        layer.update(multi_plane_ffn_norm=True, ffn_cfgs=dict(type='MultiPlaneFFN', feedforward_channels=ff, ffn_drop=drop),
                     norm_cfg=dict(type='MultiPlaneNorm', norm_cfg=dict(type='LN')))
    built = {}
    for name, cfg in (('shared', base), ('multi_plane', mp_cfg)):
        torch.manual_seed(2)
        lifter, encoder, _, _ = hc.build(cfg, d)
        built[name] = (lifter, encoder)
    metas, feats, _ = hc.frame_inputs(base, 'nuscenes_occ', d, seed=0, want_images=False)
    dirs = [torch.randn(1, n, C, generator=g).to(d) for n in SIZES]

    def frame(name, train):
        lifter, encoder = built[name]

        def run():
            with torch.set_grad_enabled(train):
                rep = encoder(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
                if train:
                    loss = sum((o * w).sum() for o, w in zip(rep, dirs))
                    torch.autograd.grad(loss, [p for p in encoder.parameters() if p.requires_grad], allow_unused=True)
        return run

    for mode in ('inference', 'training'):
        for lifter, encoder in built.values():
            encoder.train(mode == 'training'); lifter.train(mode == 'training')
        res = {k: summarise(v) for k, v in measure({k: frame(k, mode == 'training') for k in built}).items()}
        emit(dict(step='encoder', config='nuscenes_occ', mode=mode, iters=args.iters, repeats=args.repeats,
                  multi_plane_over_shared=round(res['multi_plane']['median_ms'] / res['shared']['median_ms'], 4), **res))

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write("\n".join(lines) + "\n")
