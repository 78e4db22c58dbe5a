"""Kernel-level A/B of the one-product bfloat16 mode of the tall-Linear kernels (SO_LINEAR_BF16X1, ``bf16=True``) against the default
(the exact three-way split) on ONE layer's twelve projections — sampling_offsets, attention_weights and value / output projections
of the self- and the two cross-attentions, the stacked value projection of the camera features, the two FFN Linears — at the TPV
sizes of the shipped nuscenes_depth (257 x 257 x 31) and nuscenes_occ (257 x 257 x 25) configs; the camera-feature rows (178 500)
are those of scripts/bench_linear.py for both.  Forward (with bias), input gradient and weight / bias gradient.

Method: the two modes alternate inside every round; a round times REPS back-to-back calls of one mode between two
device events; 3 warm-up rounds, then the median and the min - max of 10 rounds; garbage collection off; random N(0, 1) data.
One JSON line per (config, projection, pass) to --out (default profiles/linear_bf16_bench.jsonl), a summary line at the end."""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from selfocc_amd.linear import linear_fwd, linear_dgrad, linear_wgrad, dgrad_supported  # noqa: E402

REPS, ROUNDS, WARM = 10, 10, 3


def layer(hw, zh, cam=178500):
    s = hw + 2 * zh
    return [("self_off", s, 96, 432), ("self_aw", s, 96, 216), ("self_val", s, 96, 96), ("self_out", s, 96, 96),
            ("hw_off", hw, 96, 384), ("hw_aw", hw, 96, 192), ("hw_out", hw, 96, 96),
            ("zh_off", zh, 96, 2304), ("zh_aw", zh, 96, 1152), ("cross_val_x3", cam, 96, 288),
            ("ffn1", s, 96, 192), ("ffn2", s, 192, 96)]


CONFIGS = {"nuscenes_depth": layer(257 * 257, 31 * 257), "nuscenes_occ": layer(257 * 257, 25 * 257)}


def time_pair(fn):
    """fn(bf16) -> us per call of (default, flagged): alternating inside every round"""
    t = {False: [], True: []}
    for r in range(WARM + ROUNDS):
        for mode in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn(mode)
            e1.record()
            e1.synchronize()
            if r >= WARM:
                t[mode].append(e0.elapsed_time(e1) * 1e3 / REPS)
    return {m: dict(med=statistics.median(v), min=min(v), max=max(v)) for m, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "linear_bf16_bench.jsonl"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    d = torch.device("cuda:0")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    gc.disable()
    g = torch.Generator(device=d).manual_seed(0)
    rows, tot = [], {}
    with open(a.out, "w") as f:
        for cfg in a.configs.split(","):
            for name, T, K, N in CONFIGS[cfg]:
                x = torch.randn(T, K, device=d, generator=g)
                w = torch.randn(N, K, device=d, generator=g) / K ** 0.5
                b = torch.randn(N, device=d, generator=g)
                dy = torch.randn(T, N, device=d, generator=g)
                y = torch.empty(T, N, device=d)
                passes = {"fwd": lambda m: linear_fwd(x, w, b, out=y, bf16=m), "wgrad": lambda m: linear_wgrad(dy, x, bf16=m)}
                if dgrad_supported(T, N, K):
                    passes["dgrad"] = lambda m: linear_dgrad(dy, w, bf16=m)
                for p, fn in passes.items():
                    r = time_pair(fn)
                    row = dict(config=cfg, proj=name, T=T, K=K, N=N, **{"pass": p}, default_us=round(r[False]["med"], 2),
                               default_min=round(r[False]["min"], 2), default_max=round(r[False]["max"], 2),
                               bf16_us=round(r[True]["med"], 2), bf16_min=round(r[True]["min"], 2), bf16_max=round(r[True]["max"], 2),
                               ratio=round(r[True]["med"] / r[False]["med"], 3),
                               slower_beyond_spread=bool(r[True]["med"] > r[False]["max"]))
                    rows.append(row)
                    f.write(json.dumps(row) + "\n")
                    f.flush()
                    k = (cfg, p)
                    tot[k] = [tot.get(k, [0, 0])[0] + r[False]["med"], tot.get(k, [0, 0])[1] + r[True]["med"]]
                    print(json.dumps(row), flush=True)
                del x, w, b, dy, y
        summ = dict(summary={f"{c}.{p}": dict(default_us=round(v[0], 1), bf16_us=round(v[1], 1), ratio=round(v[1] / v[0], 3))
                             for (c, p), v in tot.items()},
                    slower_beyond_spread=[f"{r['config']}.{r['proj']}.{r['pass']}" for r in rows if r["slower_beyond_spread"]])
        f.write(json.dumps(summ) + "\n")
        print(json.dumps(summ))


if __name__ == "__main__":
    main()
