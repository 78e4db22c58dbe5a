"""Shared by tests/test_multi_plane_cpu.py and tests/test_multi_plane_gpu.py: the reference-generated fixtures of
tests/golden/make_golden_multi_plane.py (MultiPlaneFFN / MultiPlaneNorm and the TPV encoder with multi_plane_ffn_norm=True),
loaded once, and our modules built on them."""
import copy
import functools
import glob
import importlib.util
import json
import os

import numpy as np
import torch

from util import seeded_fill

G = os.path.join(os.path.dirname(__file__), "golden")
PLANES = ('out_hw', 'out_zh', 'out_wz')


@functools.lru_cache(None)
def cfg():
    return json.load(open(os.path.join(G, "encoder_full_mp_cfg.json")))


@functools.lru_cache(None)
def generator(name="make_golden_multi_plane"):
    """the generator module, for the seeded inputs it shares with the tests (it does not touch the reference on import)"""
    spec = importlib.util.spec_from_file_location(name + "_inputs", os.path.join(G, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(None)
def load(stem):
    """<stem>.npz and its <stem>_grads_K.npz as one read-only dict"""
    out = {}
    files = [os.path.join(G, stem + ".npz")] + sorted(glob.glob(os.path.join(G, stem + "_grads_[0-9]*.npz")))
    for f in files:
        with np.load(f) as z:
            for k in z.files:
                assert k not in out, k
                out[k] = z[k]
                out[k].setflags(write=False)
    return out


def module_state(z, which):
    pre = f'param.{which}.'
    return {k[len(pre):]: torch.tensor(v) for k, v in z.items() if k.startswith(pre)}


def build_modules(device='cpu'):
    """our MultiPlaneFFN(32, 64) and MultiPlaneNorm(32, LN) through the registry / build_norm_layer, carrying the fixture's
    state dict (strict), in eval mode (dropout off, as the generator ran them)"""
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    from selfocc_amd.model.bricks import build_norm_layer
    spec = cfg()['modules']
    z = load('multi_plane_modules')
    ffn = MODELS.build(dict(type='MultiPlaneFFN', embed_dims=spec['dim'], feedforward_channels=spec['hidden'], ffn_drop=0.1))
    norm = build_norm_layer(dict(type='MultiPlaneNorm', norm_cfg=dict(type='LN')), spec['dim'])[1]
    ffn.load_state_dict(module_state(z, 'ffn'), strict=True)
    norm.load_state_dict(module_state(z, 'norm'), strict=True)
    return z, ffn.to(device).eval(), norm.to(device).eval()


def run_modules(z, ffn, norm, case, device='cpu'):
    """the generator's pass: norm(ffn(x, identity)), the scalar sum_p (out_p * dir_p).sum() and its gradients by fixture key"""
    xs = [torch.tensor(z[f'x.{p}']).to(device).requires_grad_(True) for p in range(3)]
    ids = [torch.tensor(z[f'identity.{p}']).to(device).requires_grad_(True) for p in range(3)] if case == 'id' else None
    dirs = [torch.tensor(z[f'dir.{p}']).to(device) for p in range(3)]
    mid = ffn(xs, ids)
    out = norm(mid)
    loss = sum((o * d).sum() for o, d in zip(out, dirs))
    params = [(f'param.ffn.{n}', p) for n, p in ffn.named_parameters()] + [(f'param.norm.{n}', p) for n, p in norm.named_parameters()]
    names = [n for n, _ in params] + [f'x.{p}' for p in range(3)] + ([f'identity.{p}' for p in range(3)] if ids else [])
    grads = torch.autograd.grad(loss, [p for _, p in params] + xs + (ids or []))
    got = {f'{case}.grad.{n}': g for n, g in zip(names, grads)}
    for p in range(3):
        got[f'{case}.ffn.{p}'] = mid[p].detach()
        got[f'{case}.norm.{p}'] = out[p].detach()
    return got


def rel_err(got, ref):
    ref = torch.tensor(np.array(ref))
    return float((got.detach().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def setup_encoder_cpu(variant):
    """variant 'post' / 'pre': our encoder + lifter at the fixture's config with parameters and inputs regenerated from the
    seeds, checked against the generator's checksums"""
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    c = cfg()
    z = load('encoder_full_mp' if variant == 'post' else 'encoder_full_mp_prenorm')
    spec = c['spec' if variant == 'post' else 'spec_prenorm']
    torch.manual_seed(0)
    enc = MODELS.build(dict(type='TPVFormerEncoder', **copy.deepcopy(c['encoder' if variant == 'post' else 'encoder_prenorm'])))
    enc.init_weights()
    lifter = MODELS.build(dict(type='TPVQueryLifter', **c['lifter']))
    seeded_fill(enc, spec['seed_params'])
    seeded_fill(lifter, spec['seed_lifter'])
    feats, l2i, loss_dirs = generator("make_golden").full_encoder_inputs(spec)
    chk = [sum(float(p.detach().double().sum()) for p in enc.parameters()), sum(float(p.detach().double().abs().sum()) for p in enc.parameters())]
    assert np.allclose(chk, z['check.enc'], rtol=1e-9), "seeded parameters differ from the generator's (torch RNG changed?)"
    assert np.allclose([sum(float(p.detach().double().sum()) for p in lifter.parameters())], z['check.lift'], rtol=1e-9)
    assert np.allclose([float(f.double().sum()) for f in feats], z['check.feats'], rtol=1e-9)
    assert np.array_equal(l2i, z['lidar2img'])
    return z, spec, enc, lifter, feats, l2i, loss_dirs
