"""GPU: every instantiation of the render backward (render_bwd_kernel: row type x (M, WPR) x scatter x mapping kind) and of the
sample-parallel training forward it differentiates (render_fwd_samples_kernel) against float64 autograd of the torch port, at
the bounds of the training-shape test (TRAIN_SHAPE_TOL) instead of the loose 2e-3 / 2e-2 / 5e-2 of the older tests.

Case table, reference, mask and metrics: tests/render_bwd_cases.py.  What makes the bounds trustworthy (the float32 port stays
a factor 5 below them, deliberately defective gradients a factor 2 above): tests/test_render_bwd_cases_cpu.py.  Every case
appends its measured figures to render_bwd_sharp.jsonl next to the training-shape test's log (one full run:
profiles/render_bwd_sharp_parity.jsonl)."""
import json
import os

import pytest
import torch

import render_bwd_cases as rc
from selfocc_amd import abi, synthetic as sy
from selfocc_amd.render import RaySet, render_rays_autograd
from test_render_bwd_gpu import LOG as TRAIN_SHAPE_LOG

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(TRAIN_SHAPE_LOG), "render_bwd_sharp.jsonl")


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_render_forward_and_backward_vs_float64_autograd(hip, case):
    r = rc.reference(case)
    inp = r.inp
    inp.cfg.bwd_scatter = case.scatter
    v = inp.vol.to(D0)
    sdf_p = v.sdf.clone().requires_grad_(True)
    feat_p = None if v.feat is None else v.feat.clone().requires_grad_(True)
    inv_s = torch.tensor([inp.cfg.inv_s], device=D0, requires_grad=True)
    ex = inp.ex
    out = render_rays_autograd(v.with_tensors(sdf_p, feat_p), inv_s,
                               RaySet(origins=ex.origins.to(D0), dirs=ex.dirs.to(D0), dir_norm=ex.dir_norm.to(D0)), inp.cfg,
                               want_grad_samples=True, t_rand=None if inp.t_rand is None else inp.t_rand.to(D0),
                               bkgd_rays=None if inp.bk is None else inp.bk.to(D0))
    sum((out[k] * r.G[k].to(D0)).sum() for k in r.G).backward()
    got = dict(g_sdf=sdf_p.grad.cpu().double(), g_inv_s=inv_s.grad.cpu().double()[0],
               g_feat=None if feat_p is None else feat_p.grad.cpu().double()[..., :inp.n_ch])
    m = rc.grad_metrics(got, r.grads)
    m.update(rc.forward_metrics({k: out[k].detach().cpu() for k in r.G}, r))
    rec = dict(case=rc.case_id(case), row=rc.row_label(case.row), lane_shape=list(rc.lane_shape(case.S)), scatter=case.scatter,
               mapping=case.mapping, jitter=case.jitter, sample_pos=case.sample_pos, n_rays=ex.n_rays, n_samples=case.S,
               rays_with_upstream=r.keep.float().mean().item(), **m)
    print("\n" + json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    b = rc.bounds(case)
    for k, val in m.items():
        assert val <= b[k], (k, val, b[k], rec)
    if feat_p is not None:
        assert r.grads['g_feat'].abs().max() > 0
        assert feat_p.grad.dtype == feat_p.dtype
        if feat_p.shape[-1] > inp.n_ch:
            assert feat_p.grad[..., inp.n_ch:].abs().max() == 0          # the pad channels of masked and SH rows: exactly 0


def test_more_than_512_samples_is_refused_and_nothing_is_launched(hip):
    """S = 513 = 64 kMaxM + 1: selfocc_render_bwd returns an error code with the limit in selfocc_last_error"""
    from selfocc_amd._lib import lib, ptr, current_stream
    from selfocc_amd.render import marshal_render_args
    vol = sy.make_volume("cfg1", n_rgb=3, n_sem=5, seed=2).to(D0)
    ex = sy.explicit_rays(sy.make_rays("cfg1", seed=2))
    rg = RaySet(origins=ex.origins.to(D0), dirs=ex.dirs.to(D0), dir_norm=ex.dir_norm.to(D0))
    cfg = sy.make_render_config("cfg1")
    cfg.n_samples = 513
    a, _out, _keep = marshal_render_args(vol, rg, cfg, outputs={})
    ba = abi.SoRenderBwdArgs()
    ba.fwd = a
    g_depth, g_weights = torch.ones(rg.n_rays, device=D0), torch.ones(rg.n_rays, 513, device=D0)
    g_sdf_vol, g_feat, g_inv_s = torch.zeros_like(vol.sdf), torch.zeros_like(vol.feat), torch.zeros(1, device=D0)
    ba.g_depth, ba.g_weights, ba.g_sdf_vol, ba.g_feat_vol, ba.g_inv_s = ptr(g_depth), ptr(g_weights), ptr(g_sdf_vol), ptr(g_feat), ptr(g_inv_s)
    assert lib().selfocc_render_bwd(ba, current_stream(D0)) < 0
    assert b"n_samples must be <=" in lib().selfocc_last_error()
    torch.cuda.synchronize()
    assert g_sdf_vol.abs().max() == 0 and g_feat.abs().max() == 0 and g_inv_s.abs().max() == 0
    a.n_samples = 512                                                     # the same arguments at the limit run
    ba.fwd = a
    assert lib().selfocc_render_bwd(ba, current_stream(D0)) == 0
    torch.cuda.synchronize()
    assert g_sdf_vol.abs().max() > 0
